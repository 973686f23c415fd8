"""rf_topk_multi_f64 / BatchComparator.topk_multi with f64 scores on the device: every row equals, `==` on float64 with no tolerance, the ranking of the
oracle's per-candidate scores -- NaN dropped, ordered by (score, index), the first k -- and equals topk() of the same comparator.  The corpora are the four
of tests/test_gpu_topk_multi.py (a padded last tile, a single length 20, ragged 0..64 with exact and mixed tiles and empty candidates, `char` symbols)
and a fifth, ragged one with planted CROSS-LENGTH ties: candidates of different lengths -- different maxima, different tiles -- whose dist / maximum is
the same number, which the 32-bit score image (rf_norm_key.hpp) must give one key and the index must order.

The ties of the fifth corpus, for its 20-symbol query.  (A candidate of 40 symbols is at least 20 edits away from a query of 20, so "length 20 at 5
edits, length 40 at 10 edits" cannot tie for any metric here; the lengths below are the ones at which the ratios do meet.)
    A  length 20, 4 substitutions   levenshtein / lcs_seq 4 / 20, indel 8 / 40            = 0.2
    B  length 25, 5 insertions      levenshtein / lcs_seq 5 / 25 = 0.2, indel 5 / 45
    C  length 30, 10 insertions     indel 10 / 50 = 0.2, levenshtein / lcs_seq 10 / 30
Six rows are closer than 0.2 (copies, 1..3 substitutions); 12 rows of A, 8 of B, 12 of C: for levenshtein and lcs_seq A and B tie (20 rows, two
lengths) from rank 7 on, for indel B comes first and A and C tie (24 rows, two lengths) from rank 15 on -- either way the 16th score is tied across
lengths by more rows than the first 16 hold.  test_the_cross_length_ties_are_there asserts that from the oracle alone.

Which road a list took is read from RF_TRACE_PLAN in child processes (tests/topk_multi_f64_check.py)."""
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
from test_gpu_topk_multi import LISTS, QLEN, Case, case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel, "lcs_seq": rf.distance.lcs_seq, "osa": rf.distance.osa,
       "damerau_levenshtein": rf.distance.damerau_levenshtein, "jaro": rf.distance.jaro, "jaro_winkler": rf.distance.jaro_winkler}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel, "lcs_seq": o.lcs_seq, "osa": o.osa, "jaro": o.jaro, "jaro_winkler": o.jaro_winkler}
INDEL_RATIO = rf.Args().ratio_indel_normalization()


class TieCase(Case):
    """the fifth corpus (module docstring): ragged, lengths 20 / 25 / 30 / 64 in exact tiles and everything else in mixed ones"""

    def __init__(self):
        rng = np.random.default_rng(5)
        self.kind = "e"
        alphabet = [bytes([c]) for c in range(48, 122)]
        rand = lambda ln: b"".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=ln))  # noqa: E731
        self.queries = {name: rand(ln) for name, ln in QLEN.items()}
        n = 2503
        lens = [int(x) for x in np.where(rng.random(n) < 0.5, rng.choice([20, 25, 30, 64], size=n), rng.integers(0, 65, size=n))]
        cands = [rand(ln) for ln in lens]
        q = self.queries["20"]

        def substituted(edits):
            row = bytearray(q)
            for pos in rng.choice(len(row), size=edits, replace=False):
                row[int(pos)] = ord("~")  # a symbol no query and no random candidate holds
            return bytes(row)

        def inserted(extra):
            row = [bytes([c]) for c in q]
            for _ in range(extra):
                row.insert(int(rng.integers(0, len(row) + 1)), b"~")
            return b"".join(row)

        planted = [substituted(0), substituted(0), substituted(1), substituted(2), substituted(3), substituted(3)]
        planted += [substituted(4) for _ in range(12)] + [inserted(5) for _ in range(8)] + [inserted(10) for _ in range(12)]
        order = rng.permutation(len(planted))
        at, stride = 11, 37  # no multiple of a tile: equal scores land in different tiles and different wavefronts' ranges
        for j in order:
            cands[at % n] = planted[int(j)]
            at += stride
        # a few near-copies of the other queries as well, so that every list has a ranking worth the name
        for name, qq in self.queries.items():
            if name != "20":
                cands[at % n] = qq
                at += stride
        self.cands, self.n = cands, n
        self.corpus = rf.Corpus.from_list(cands)
        self.ren = lambda s: s
        self.data, self.offsets = rf.ragged(cands)
        self._bc = {}


@functools.lru_cache(maxsize=None)
def fcase(kind):
    return TieCase() if kind == "e" else case(kind)


def comparator(c, metric, name):
    key = (metric, name)
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
        v.setflags(write=False)
        _scores[key] = v
    return _scores[key]


def descending(op):
    return op in (N.OP_SIMILARITY, NS)


def expected(c, metric, name, op, k, cutoff=None, weights=None, base=0):
    s = scores(c, metric, name, op, cutoff, weights)
    idx = np.nonzero(~np.isnan(s))[0]
    v = s[idx]
    order = np.lexsort((idx, -v if descending(op) else v))[:k]
    return v[order], (idx[order] + base).astype(np.uint64)


_single = {}


def single(c, metric, name, op, k, cutoff, weights, base, args):
    key = (c.kind, metric, name, op, k, cutoff, weights, base)
    if key not in _single:
        _single[key] = comparator(c, metric, name).topk(c.corpus, k, op, args=args, index_base=base, score_cutoff=cutoff, weights=weights)
    return _single[key]


def check_list(c, members, k, op, cutoff=None, weights=None, base=0):
    """members: (metric, query name) pairs; "ratio" / "ratio_indel" are fuzz::RatioBatchComparator without / with RF_FLAG_RATIO_INDEL_NORMALIZATION.
    Every row against the oracle's ranking and against topk() of the same comparator, bit for bit."""
    args = INDEL_RATIO if any(m == "ratio_indel" for m, _ in members) else None
    cls = type(comparator(c, *members[0]))
    got = cls.topk_multi([comparator(c, m, name) for m, name in members], c.corpus, k, op, args=args, index_base=base, score_cutoff=cutoff, weights=weights)
    assert len(got) == len(members)
    for (metric, name), (s, i) in zip(members, got):
        what = (c.kind, metric, name, k, op, cutoff, weights)
        es, ei = expected(c, metric, name, op, k, cutoff, weights, base)
        assert s.dtype == np.float64 and i.dtype == np.uint64
        assert len(s) == len(es) and (s == es).all() and i.tolist() == ei.tolist(), what
        ss, si = single(c, metric, name, op, k, cutoff, weights, base, args)
        assert len(s) == len(ss) and (s == ss).all() and i.tolist() == si.tolist(), what
    return got


@pytest.mark.parametrize("k", [1, 16, 64, 65])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e"])
def test_rows_equal_the_oracle_ranking_and_topk(kind, k):
    c = fcase(kind)
    for names in LISTS.values():
        for op in (ND, NS):
            check_list(c, [("levenshtein", name) for name in names], k, op)


def test_the_cross_length_ties_are_there():
    """from the oracle alone: in corpus (e) more rows are tied at the 16th score than the first 16 hold of them, and the tied rows span at least two
    candidate lengths -- for every fused family and both ops"""
    c = fcase("e")
    lens = np.diff(c.offsets.astype(np.int64))
    for metric in ("levenshtein", "indel", "lcs_seq", "ratio", "ratio_indel"):
        for op in (NS,) if metric.startswith("ratio") else (ND, NS):
            s = scores(c, metric, "20", op)
            es, _ = expected(c, metric, "20", op, 16)
            tied = np.nonzero(s == es[-1])[0]
            assert len(tied) > int((es == es[-1]).sum()) >= 1, (metric, op)
            assert len(set(lens[tied].tolist())) >= 2, (metric, op, sorted(set(lens[tied].tolist())))


@pytest.mark.parametrize("kind", ["a", "b", "c", "d", "e"])
@pytest.mark.parametrize("metric", ["indel", "lcs_seq", "ratio", "ratio_indel"])
def test_lcs_family_and_ratio_groups(kind, metric):
    c = fcase(kind)
    for op in (N.OP_SIMILARITY, NS) if metric.startswith("ratio") else (ND, NS):
        check_list(c, [(metric, name) for name in LISTS[7]], 16, op)
        check_list(c, [(metric, name) for name in LISTS[4]], 64, op)


@pytest.mark.parametrize("kind", ["a", "c", "e"])
@pytest.mark.parametrize("weights", [None, (1, 2, 3), (2, 2, 5), (2, 2, 2)])
def test_mixed_metrics(kind, weights):
    """one list over every metric with a normalized op: levenshtein, indel and lcs_seq pair up within their families; jaro, jaro_winkler, osa and
    damerau_levenshtein go per query; under (1, 2, 3) the levenshtein queries go per query as well, under (2, 2, 5) they run as Indel x 2"""
    c = fcase(kind)
    members = [("levenshtein", "64"), ("indel", "64"), ("jaro", "20"), ("lcs_seq", "20"), ("osa", "64"), ("damerau_levenshtein", "20"), ("levenshtein", "64b"),
               ("jaro_winkler", "33"), ("indel", "33"), ("lcs_seq", "32"), ("osa", "20"), ("levenshtein", "20"), ("levenshtein", "1")]
    for op in (ND, NS):
        check_list(c, members, 16, op, weights=weights)


@pytest.mark.parametrize("kind", ["a", "e"])
def test_weights_beyond_the_key_and_zero_weights(kind):
    """(1024, 1024, 1024): the maximum exceeds 65535, so the list goes per query -- with the same rows; (0, 0, 0): every distance and every maximum is 0,
    every normalized distance 0.0, and the index alone orders"""
    c = fcase(kind)
    lev = [("levenshtein", name) for name in LISTS[7]]
    for op in (ND, NS):
        check_list(c, lev, 16, op, weights=(1024, 1024, 1024))
        check_list(c, lev, 16, op, weights=(0, 0, 0))
    got = check_list(c, lev, 16, ND, weights=(0, 0, 0))
    for s, i in got:
        assert (s == 0.0).all() and i.tolist() == list(range(16))


@pytest.mark.parametrize("kind", ["a", "c", "e"])
def test_cutoffs(kind):
    """a loose cutoff (normalized_similarity >= 0.3: the fused kernel's own None rule; few rows pass, so count < k) and a tight one (>= 0.9: the per-query
    early-out road); the same for normalized_distance"""
    c = fcase(kind)
    lev = [("levenshtein", name) for name in LISTS[7]]
    for k in (16, 64):
        got = check_list(c, lev, k, NS, cutoff=0.3)
        if k == 64 and kind != "e":  # only the planted rows of a 64-symbol query come that close to it
            assert all(0 < len(s) < k for (_, name), (s, _) in zip(lev, got) if QLEN[name] == 64)
        check_list(c, lev, k, NS, cutoff=0.9)
        check_list(c, lev, k, ND, cutoff=0.7)
        check_list(c, lev, k, ND, cutoff=0.1)
        for metric in ("indel", "ratio", "ratio_indel"):
            check_list(c, [(metric, name) for name in LISTS[4]], k, NS, cutoff=0.3)
            check_list(c, [(metric, name) for name in LISTS[4]], k, NS, cutoff=0.9)
    got = check_list(c, lev, 64, ND, cutoff=0.0)
    if kind != "e":
        assert all(len(s) == 2 for (_, name), (s, _) in zip(lev, got) if QLEN[name] == 64)  # the two copies


def test_k_beyond_the_corpus_and_index_base():
    c = fcase("b")
    got = check_list(c, [("levenshtein", name) for name in LISTS[5]], c.n + 5, ND)
    assert all(len(s) == c.n for s, _ in got)
    base = 2**40 + 5
    for kind in ("a", "c", "e"):
        got = check_list(fcase(kind), [("levenshtein", name) for name in LISTS[7]], 16, NS, base=base)
        assert all(int(i.min()) >= base for _, i in got)
        check_list(fcase(kind), [("indel", name) for name in LISTS[4]], 65, NS, base=base)
        check_list(fcase(kind), [("ratio", name) for name in LISTS[4]], 16, N.OP_SIMILARITY, base=base)
    # fewer candidates than k on the fused road: count = n
    tiny = rf.Corpus.from_list([b"abcd", b"abce", b"", b"xbcd", b"abcd"])
    lev = rf.distance.levenshtein.BatchComparator
    got = lev.topk_multi([lev(q) for q in (b"abcd", b"abc")], tiny, 16, ND)
    assert [(s.tolist(), i.tolist()) for s, i in got] == [([0.0, 0.0, 0.25, 0.25, 1.0], [0, 4, 1, 3, 2]), ([0.25, 0.25, 0.25, 0.5, 1.0], [0, 1, 4, 3, 2])]


def test_the_default_op_of_a_float_class_is_similarity():
    c = fcase("b")
    ratio = rf.fuzz.RatioBatchComparator
    cs = [comparator(c, "ratio", name) for name in LISTS[4]]
    got = ratio.topk_multi(cs, c.corpus, 16)
    for (s, i), name in zip(got, LISTS[4]):
        es, ei = expected(c, "ratio", name, NS, 16)
        assert s.dtype == np.float64 and (s == es).all() and i.tolist() == ei.tolist()


def test_errors_and_empty_inputs_on_the_device():
    c = fcase("b")
    lev = rf.distance.levenshtein.BatchComparator
    assert lev.topk_multi([], c.corpus, 4, NS) == []
    with pytest.raises(rf.RfError) as e:
        lev.topk_multi([comparator(c, "levenshtein", "20")], c.corpus, 0, NS)
    assert e.value.status == N.RF_ERR_INVALID_ARG
    with pytest.raises(rf.RfError) as e:  # a distance op of the ratio
        lev.topk_multi([comparator(c, "levenshtein", "20"), comparator(c, "ratio", "20")], c.corpus, 4, ND)
    assert e.value.status == N.RF_ERR_INVALID_ARG
    empty = rf.Corpus.from_list([])
    got = lev.topk_multi([comparator(c, "levenshtein", "20"), comparator(c, "levenshtein", "20b")], empty, 4, NS)
    assert [len(s) for s, _ in got] == [0, 0]


@pytest.mark.parametrize("missing", ["out_score", "out_index"])
def test_a_null_row_array_over_a_non_empty_corpus_writes_nothing(missing):
    c = fcase("b")
    cs = [comparator(c, "levenshtein", "20"), comparator(c, "levenshtein", "20b")]
    hs = (C.c_void_p * 2)(*[x._h for x in cs])
    args = rf.Args().to_c(True)
    score, index, count = np.full((2, 4), 77.0), np.full((2, 4), 77, dtype=np.uint64), np.full(2, 77, dtype=np.uint32)
    st = N.lib().rf_topk_multi_f64(hs, 2, c.corpus._h, NS, C.byref(args), 4, 0, None if missing == "out_score" else score.ctypes.data,
                                   None if missing == "out_index" else index.ctypes.data, count.ctypes.data, None)
    assert st == N.RF_ERR_INVALID_ARG
    assert (count == 77).all() and (score == 77.0).all() and (index == 77).all()


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "topk_multi_f64_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_roads_by_the_plan_trace():
    """a child process with RF_TRACE_PLAN: fused groups of 4 and 2 for both ops, the ratio, weights (2, 2, 2) / (2, 2, 5) / (0, 0, 0) and a loose cutoff;
    per query for (1, 2, 3), (1024, 1024, 1024), a tight cutoff, k = 65 and the f64 / OSA / Damerau members of a mixed list; with RF_TOPK_MULTI=0 every
    list per query -- with the same rows"""
    r = _child("roads")
    assert "roads ok" in r.stdout, r.stdout[-2000:]
    r = _child("roads_off", RF_TOPK_MULTI="0")
    assert "roads_off ok" in r.stdout, r.stdout[-2000:]


def test_several_tiles_per_wavefront():
    """tests/topk_multi_f64_check.py with one workgroup per CU and a sample of 8 tiles: every wavefront of the fused kernel owns at least 3 tiles, the
    last a partial one; single-length and ragged corpora; the checker asserts from the plan lines that groups of 4 ran fused and that the sample pass ran"""
    r = _child("multitile", RF_SCAN_BLOCKS_PER_CU="1", RF_TOPK_SAMPLE="8")
    assert "FAILURES 0" in r.stdout, r.stdout[-3000:]
