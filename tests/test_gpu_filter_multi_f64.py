"""rf_filter_multi_f64 / BatchComparator.filter_multi with f64 scores on the device: every row equals the oracle's per-candidate float64 values under the same
cutoff with the NaNs dropped -- the same indices, the same doubles as 64-bit patterns, in the order asked for -- and equals filter_many() of the same
comparator.  The corpora are the four of tests/test_gpu_filter_multi.py (a padded last tile, a single length 20, ragged 0..64 with exact and mixed tiles and
empty candidates, `char` symbols; per query 2 copies, rows at 1 / 2 / 3 edits and prefix sharers that survive the looks at columns 8 and 16 and die later) and
the ragged corpus of tests/test_gpu_topk_multi_f64.py with its CROSS-LENGTH ties: for the 20-symbol query, rows of length 20 with 4 substitutions, of length
25 = the query + 5 inserted symbols and of length 30 = the query + 10 inserted symbols, so that 4 / 20 = 5 / 25 (levenshtein, lcs_seq) and 8 / 40 = 10 / 50
(indel) are one normalized distance from two maxima, in different tiles.

Cutoffs: normalized_similarity >= 0.9 and normalized_distance <= 0.1 are tight (plan() sets `early`: the fused road), normalized_similarity >= 0.2 is loose
and no cutoff is none (both per query).  Which road a list took is read from RF_TRACE_PLAN in child processes (tests/filter_multi_f64_check.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from oracle import oracle as o

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dl_reference as R  # noqa: E402
from test_gpu_filter_multi import LISTS, QLEN, case  # noqa: E402
from test_gpu_topk_multi_f64 import TieCase  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel, "lcs_seq": rf.distance.lcs_seq, "osa": rf.distance.osa,
       "damerau_levenshtein": rf.distance.damerau_levenshtein, "jaro": rf.distance.jaro, "jaro_winkler": rf.distance.jaro_winkler}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel, "lcs_seq": o.lcs_seq, "osa": o.osa, "jaro": o.jaro, "jaro_winkler": o.jaro_winkler}
ORDERS = (N.FILTER_BY_INDEX, N.FILTER_BY_SCORE, N.FILTER_ANY)
INDEL_RATIO = rf.Args().ratio_indel_normalization()


@functools.lru_cache(maxsize=None)
def fcase(kind):
    if kind != "e":
        return case(kind)
    c = TieCase()
    c.kind = "tie"  # (this module's caches are keyed by it)
    return c


def comparator(c, metric, name):
    key = ("f64", metric, name)
    if key not in c._bc:
        cls = rf.fuzz.RatioBatchComparator if metric.startswith("ratio") else GPU[metric].BatchComparator
        c._bc[key] = cls(c.queries[name])
    return c._bc[key]


_scores = {}


def scores(c, metric, name, op, cutoff=None, weights=None):
    """the oracle's per-candidate float64 values, NaN = None; computed once per question, never changed"""
    key = (c.kind, metric, name, op, cutoff, weights)
    if key not in _scores:
        q = c.ren(c.queries[name])
        kw = {}
        if cutoff is not None:
            kw["score_cutoff"] = cutoff
        if metric == "damerau_levenshtein":
            if not hasattr(c, "_rows"):
                c._rows = R.ragged_rows(c.data, c.offsets)
            v = R.ops(op, q, c._rows[0], c._rows[1], cutoff)
        elif metric == "ratio":  # fuzz.rs:141: the inner lcs_seq comparator's normalization
            v = o.fuzz.RatioBatchComparator(q).many(NS, c.data, c.offsets, nthreads=8, **kw)
        elif metric == "ratio_indel":  # the documented ratio
            v = o.indel.BatchComparator(q).many(NS, c.data, c.offsets, nthreads=8, **kw)
        else:
            if weights is not None and metric == "levenshtein":
                kw["weights"] = weights
            v = ORA[metric].BatchComparator(q).many(op, c.data, c.offsets, nthreads=8, **kw)
        v = np.asarray(v, dtype=np.float64)
        v.setflags(write=False)
        _scores[key] = v
    return _scores[key]


def descending(op):
    return op in (N.OP_SIMILARITY, NS)


def expected(c, metric, name, op, order, cutoff=None, weights=None, base=0):
    """(indices, scores) of the oracle's Somes: ascending index, or best score first with ties by index"""
    s = scores(c, metric, name, op, cutoff, weights)
    idx = np.nonzero(~np.isnan(s))[0]
    if order == N.FILTER_BY_SCORE:
        v = s[idx]
        idx = idx[np.lexsort((idx, -v if descending(op) else v))]
    return (idx + base).astype(np.uint64), s[idx]


_single = {}


def single(c, metric, name, op, order, cutoff, weights, base, args):
    key = (c.kind, metric, name, op, order, cutoff, weights, base)
    if key not in _single:
        _single[key] = comparator(c, metric, name).filter_many(op, c.corpus, args=args, order=order, index_base=base, score_cutoff=cutoff, weights=weights)
    return _single[key]


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).tolist()


def pairs(i, s):
    return sorted(zip(i.tolist(), bits(s)))


def check_list(c, members, op, cutoff=None, weights=None, base=0, orders=ORDERS):
    """members: (metric, query name) pairs; "ratio" / "ratio_indel" are fuzz::RatioBatchComparator without / with RF_FLAG_RATIO_INDEL_NORMALIZATION.
    Every row against the oracle's Somes and against filter_many() of the same comparator, bit for bit, capacity ample."""
    args = INDEL_RATIO if any(m == "ratio_indel" for m, _ in members) else None
    cls = type(comparator(c, *members[0]))
    got = None
    for order in orders:
        got = cls.filter_multi([comparator(c, m, name) for m, name in members], op, c.corpus, args=args, order=order, index_base=base, score_cutoff=cutoff,
                               weights=weights)
        assert len(got) == len(members)
        for (metric, name), (i, s) in zip(members, got):
            what = (c.kind, metric, name, op, cutoff, weights, order)
            ei, es = expected(c, metric, name, op, order, cutoff, weights, base)
            si, ss = single(c, metric, name, op, order, cutoff, weights, base, args)
            assert i.dtype == np.uint64 and s.dtype == np.float64
            if order == N.FILTER_ANY:
                assert pairs(i, s) == pairs(ei, es) == pairs(si, ss), what
            else:
                assert i.tolist() == ei.tolist() and bits(s) == bits(es), what
                assert i.tolist() == si.tolist() and bits(s) == bits(ss), what
    return got


# ---- 1. rows equal the oracle
@pytest.mark.parametrize("op,cutoff", [(NS, 0.9), (ND, 0.1), (NS, 0.2), (NS, None), (ND, None)])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_levenshtein_rows_equal_the_oracle_and_filter_many(kind, op, cutoff):
    """similarity >= 0.9 and distance <= 0.1 run fused, similarity >= 0.2 (loose) and no cutoff go per query"""
    c = fcase(kind)
    for names in LISTS.values():
        check_list(c, [("levenshtein", name) for name in names], op, cutoff, orders=ORDERS if cutoff is not None else ORDERS[:2])


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("metric", ["indel", "lcs_seq", "ratio"])
def test_lcs_family_and_ratio_rows(kind, metric):
    c = fcase(kind)
    ops = (N.OP_SIMILARITY, NS) if metric == "ratio" else (ND, NS)
    for n in (4, 7):
        members = [(metric, name) for name in LISTS[n]]
        for op in ops:
            check_list(c, members, op, 0.1 if op == ND else 0.9, orders=ORDERS[:2])
        check_list(c, members, NS, 0.2, orders=ORDERS[:1])
    check_list(c, [(metric, name) for name in LISTS[5]], NS, None, orders=ORDERS[1:2])


def test_the_tight_cutoffs_keep_planted_rows_and_drop_the_prefix_sharers():
    """from the oracle alone, corpus (a): the 64-symbol query keeps its 2 copies + the rows at 1..3 edits under normalized_similarity >= 0.9 (6 edits allowed),
    and its 6 prefix sharers -- the query's first 24 symbols, so they survive the looks at columns 8 and 16 -- are beyond the cutoff"""
    c = fcase("a")
    s = scores(c, "levenshtein", "64", NS)
    assert int((s >= 0.9).sum()) == 2 + 20 + 3 + 3 and int((s == 1.0).sum()) == 2
    q = c.queries["64"]
    sharers = [i for i, cand in enumerate(c.cands) if cand[:24] == q[:24] and s[i] < 0.9]
    assert len(sharers) == 6


# ---- 2. the boundary: a cutoff that IS the double some row returns
BOUNDARY = [("b", "levenshtein", "20", 3 / 20), ("c", "levenshtein", "33", 3 / 33), ("a", "indel", "64", 6 / 128), ("c", "lcs_seq", "33", 3 / 33), ("b", "ratio", "20", 6 / 40)]


def boundary_cutoff(c, metric, name, op, nd):
    """the oracle's un-cut value of a row at normalized distance `nd` (a 3-edit row): the exact double, taken from its output"""
    s = scores(c, metric, name, op)
    want = nd if op == ND else 1.0 - nd
    at = np.nonzero(np.abs(s - want) < 1e-12)[0]
    assert len(at), (c.kind, metric, name, op)
    v = float(s[at[0]])
    assert (s[at] == v).all()
    return v


@pytest.mark.parametrize("kind,metric,name,nd", BOUNDARY)
def test_rows_exist_on_both_sides_of_the_boundary(kind, metric, name, nd):
    """from the oracle alone: rows AT the cutoff, rows better and rows worse than it"""
    c = fcase(kind)
    for op in (NS,) if metric == "ratio" else (ND, NS):
        s = scores(c, metric, name, op)
        v = boundary_cutoff(c, metric, name, op, nd)
        better = s > v if descending(op) else s < v
        assert int((s == v).sum()) >= 3 and int(better.sum()) >= 2 and int((~better & (s != v)).sum()) >= 100, (kind, metric, op)
        cut = scores(c, metric, name, op, v)
        assert (~np.isnan(cut)).sum() == int((s == v).sum()) + int(better.sum())  # the oracle keeps the rows at the cutoff


@pytest.mark.parametrize("kind,metric,name,nd", BOUNDARY)
def test_a_cutoff_equal_to_a_rows_score_keeps_that_row(kind, metric, name, nd):
    c = fcase(kind)
    for op in (NS,) if metric == "ratio" else (ND, NS):
        v = boundary_cutoff(c, metric, name, op, nd)
        members = [(metric, x) for x in LISTS[7]]
        got = check_list(c, members, op, v)
        i, s = got[LISTS[7].index(name)]
        assert int((s == v).sum()) >= 3  # rows at exactly the cutoff are in the row
        # ... and one ulp tighter they are not
        tighter = float(np.nextafter(v, 2.0 if descending(op) else -1.0))
        got = check_list(c, members, op, tighter, orders=ORDERS[:1])
        assert not (got[LISTS[7].index(name)][1] == v).any()


# ---- 3. cross-length ties
TIES = {"levenshtein": (20, 25), "lcs_seq": (20, 25), "indel": (20, 30)}


def test_the_cross_length_ties_are_there():
    """from the oracle alone: under normalized_distance <= 0.25 the 20-symbol query of corpus (e) has rows AT 0.2 from two candidate lengths"""
    c = fcase("e")
    lens = np.diff(c.offsets.astype(np.int64))
    for metric, (la, lb) in TIES.items():
        s = scores(c, metric, "20", ND, 0.25)
        tied = np.nonzero(s == 0.2)[0]
        assert {la, lb} <= set(lens[tied].tolist()), (metric, sorted(set(lens[tied].tolist())))
        assert int((lens[tied] == la).sum()) >= 8 and int((lens[tied] == lb).sum()) >= 8
        assert (~np.isnan(s)).sum() > len(tied)  # and rows that are closer


@pytest.mark.parametrize("metric", ["levenshtein", "lcs_seq", "indel", "ratio", "ratio_indel"])
def test_cross_length_ties_are_ordered_by_index(metric):
    c = fcase("e")
    members = [(metric, name) for name in LISTS[7]]
    if metric.startswith("ratio"):
        check_list(c, members, NS, 0.75)
        return
    got = check_list(c, members, ND, 0.25, orders=ORDERS[1:2])
    i, s = got[LISTS[7].index("20")]
    tied = i[s == 0.2]
    assert len(tied) >= 16 and tied.tolist() == sorted(tied.tolist())
    check_list(c, members, ND, 0.25)
    check_list(c, members, NS, 0.75)


# ---- 4. weights
@pytest.mark.parametrize("kind", ["a", "c", "e"])
@pytest.mark.parametrize("weights", [(2, 2, 2), (2, 2, 5), (1024, 1024, 1024), (1, 2, 3)])
def test_weights(kind, weights):
    """(2, 2, 2) and the Indel-like (2, 2, 5) run fused, (1024, 1024, 1024) -- a maximum beyond 65535 -- and (1, 2, 3) go per query (the roads:
    tests/filter_multi_f64_check.py); the rows are the oracle's either way"""
    c = fcase(kind)
    members = [("levenshtein", name) for name in LISTS[7]]
    check_list(c, members, NS, 0.9, weights=weights, orders=ORDERS[:2])
    check_list(c, members, ND, 0.1, weights=weights, orders=ORDERS[:1])


# ---- 5. a mixed list
@pytest.mark.parametrize("kind", ["a", "c", "e"])
@pytest.mark.parametrize("op,cutoff", [(NS, 0.9), (ND, 0.1)])
def test_mixed_metrics(kind, op, cutoff):
    """levenshtein, indel and lcs_seq pair up within their families; osa, damerau_levenshtein and jaro_winkler go per query"""
    c = fcase(kind)
    members = [("levenshtein", "64"), ("indel", "64"), ("jaro_winkler", "20"), ("lcs_seq", "20"), ("osa", "64"), ("damerau_levenshtein", "20"), ("levenshtein", "64b"),
               ("jaro_winkler", "33"), ("indel", "33"), ("lcs_seq", "32"), ("osa", "20"), ("levenshtein", "20"), ("levenshtein", "1")]
    check_list(c, members, op, cutoff, orders=ORDERS[:2])


# ---- 6. capacity
@pytest.mark.parametrize("capacity", [1, 3])
def test_overflow_keeps_the_true_count_and_valid_rows(capacity):
    """normalized_similarity >= 0.98 on corpus (a): the 64-symbol query has its 2 copies + 20 rows at one edit.  out_count is the true count; a row's entries
    are distinct members of the expected set, in the requested order among themselves"""
    c = fcase("a")
    lev = rf.distance.levenshtein.BatchComparator
    for n in (4, 7):
        names = LISTS[n]
        cs = [comparator(c, "levenshtein", name) for name in names]
        for order in ORDERS:
            got = lev.filter_multi(cs, NS, c.corpus, capacity=capacity, order=order, score_cutoff=0.98)
            counts = lev.last_filter_counts
            for name, (i, s), cnt in zip(names, got, counts):
                ei, es = expected(c, "levenshtein", name, NS, N.FILTER_BY_INDEX, 0.98)
                assert cnt == len(ei), (name, order)
                if name == "64":
                    assert cnt == 22
                assert len(i) == len(s) == min(cnt, capacity)
                assert len(set(i.tolist())) == len(i)
                want = dict(zip(ei.tolist(), bits(es)))
                assert all(want.get(a) == b for a, b in zip(i.tolist(), bits(s))), (name, order)
                if order == N.FILTER_BY_INDEX:
                    assert i.tolist() == sorted(i.tolist())
                elif order == N.FILTER_BY_SCORE:
                    key = list(zip((-s).tolist(), i.tolist()))
                    assert key == sorted(key)


def test_capacity_zero_is_a_pure_count():
    c = fcase("a")
    lev = rf.distance.levenshtein.BatchComparator
    for n in (4, 7):
        names = LISTS[n]
        cs = [comparator(c, "levenshtein", name) for name in names]
        for cutoff in (0.9, None):  # fused, per query
            got = lev.filter_multi(cs, NS, c.corpus, capacity=0, score_cutoff=cutoff)  # (the wrapper passes NULL row arrays)
            assert all(len(i) == 0 and len(s) == 0 for i, s in got)
            assert lev.last_filter_counts == [len(expected(c, "levenshtein", name, NS, N.FILTER_BY_INDEX, cutoff)[0]) for name in names]


# ---- 7. index_base
@pytest.mark.parametrize("kind", ["a", "c", "d"])
def test_index_base_beyond_32_bits(kind):
    c = fcase(kind)
    base = 2**40 + 5
    got = check_list(c, [("levenshtein", name) for name in LISTS[7]], NS, 0.9, base=base)
    assert any(len(i) for i, _ in got) and all(int(i.min()) >= base for i, _ in got if len(i))
    check_list(c, [("indel", name) for name in LISTS[4]], ND, 0.1, base=base, orders=ORDERS[:1])
    check_list(c, [("ratio", name) for name in LISTS[4]], N.OP_SIMILARITY, 0.9, base=base, orders=ORDERS[1:2])


# ---- 8. empty inputs, errors on the device
def test_empty_inputs():
    c = fcase("b")
    lev = rf.distance.levenshtein.BatchComparator
    assert lev.filter_multi([], NS, c.corpus, score_cutoff=0.9) == []
    empty = rf.Corpus.from_list([])
    got = lev.filter_multi([comparator(c, "levenshtein", "20"), comparator(c, "levenshtein", "20b")], NS, empty, score_cutoff=0.9)
    assert [(len(i), len(s)) for i, s in got] == [(0, 0), (0, 0)] and lev.last_filter_counts == [0, 0]
    assert got[0][1].dtype == np.float64
    with pytest.raises(rf.RfError) as e:  # a distance op of the ratio
        lev.filter_multi([comparator(c, "levenshtein", "20"), comparator(c, "ratio", "20")], ND, c.corpus, score_cutoff=0.1)
    assert e.value.status == N.RF_ERR_INVALID_ARG


def test_the_default_road_of_the_float_class():
    """fuzz.RatioBatchComparator.filter_multi with similarity as the op"""
    c = fcase("b")
    ratio = rf.fuzz.RatioBatchComparator
    cs = [comparator(c, "ratio", name) for name in LISTS[4]]
    got = ratio.filter_multi(cs, N.OP_SIMILARITY, c.corpus, order=N.FILTER_BY_SCORE, score_cutoff=0.9)
    for (i, s), name in zip(got, LISTS[4]):
        ei, es = expected(c, "ratio", name, NS, N.FILTER_BY_SCORE, 0.9)
        assert s.dtype == np.float64 and i.tolist() == ei.tolist() and bits(s) == bits(es)


# ---- 9. the ratio with and without RF_FLAG_RATIO_INDEL_NORMALIZATION
@pytest.mark.parametrize("kind", ["a", "c", "e"])
@pytest.mark.parametrize("metric", ["ratio", "ratio_indel"])
def test_ratio_normalizations(kind, metric):
    c = fcase(kind)
    for n in (4, 7):
        members = [(metric, name) for name in LISTS[n]]
        check_list(c, members, N.OP_SIMILARITY, 0.9)
        check_list(c, members, NS, 0.75, orders=ORDERS[:2])


def test_the_two_ratio_normalizations_differ_somewhere():
    """from the oracle alone: where the lengths differ -- the rows of corpus (e) with inserted symbols -- the two normalizations return different values
    under the same cutoff (5 insertions into 20 symbols: 1 - 5 / 25 against 1 - 5 / 45)"""
    c = fcase("e")
    a, b = scores(c, "ratio", "20", NS, 0.75), scores(c, "ratio_indel", "20", NS, 0.75)
    assert (~np.isnan(a)).sum() > 0 and (~np.isnan(b)).sum() > 0
    assert bits(a[~np.isnan(a)]) != bits(b[~np.isnan(b)])


@pytest.mark.parametrize("missing", ["out_score", "out_index"])
def test_a_null_row_array_with_a_capacity_writes_nothing(missing):
    c = fcase("b")
    cs = [comparator(c, "levenshtein", "20"), comparator(c, "levenshtein", "20b")]
    hs = (C.c_void_p * 2)(*[x._h for x in cs])
    args = rf.Args().score_cutoff(0.9).to_c(True)
    score, index, count = np.full((2, 4), 77.0), np.full((2, 4), 77, dtype=np.uint64), np.full(2, 77, dtype=np.uint64)
    st = N.lib().rf_filter_multi_f64(hs, 2, c.corpus._h, NS, C.byref(args), 0, 4, None if missing == "out_index" else index.ctypes.data,
                                     None if missing == "out_score" else score.ctypes.data, count.ctypes.data, N.FILTER_BY_INDEX, None)
    assert st == N.RF_ERR_INVALID_ARG
    assert (count == 77).all() and (score == 77.0).all() and (index == 77).all()


# ---- 10 / 11. roads and several tiles per wavefront: child processes
def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "filter_multi_f64_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_roads_by_the_plan_trace():
    """a child process with RF_TRACE_PLAN: a tight list of 7 queries shows fused groups [4,2] and 1 per query, for both ops, the ratio and weights (2, 2, 2) /
    (2, 2, 5); the loose, the NaN, the (1, 2, 3) and the weight-1024 lists show no fused group; with RF_FILTER_MULTI=0 every list goes per query -- with
    the same rows"""
    r = _child("roads")
    assert "roads ok" in r.stdout, r.stdout[-2000:]
    r = _child("roads_off", RF_FILTER_MULTI="0")
    assert "roads_off ok" in r.stdout, r.stdout[-2000:]


def test_several_tiles_per_wavefront():
    """tests/filter_multi_f64_check.py with one workgroup per CU: every wavefront of the fused kernel owns at least 3 tiles, the last a partial one;
    single-length and ragged corpora, 64-bit and 32-bit Levenshtein and Indel, q = 4, normalized_similarity >= 0.9, every row against the oracle's Somes; the
    checker asserts from the plan lines that groups of 4 ran fused, and on the host that tiles with and without a planted row both occur"""
    r = _child("multitile", RF_SCAN_BLOCKS_PER_CU="1")
    assert "FAILURES 0" in r.stdout, r.stdout[-3000:]
