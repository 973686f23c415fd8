"""rf_topk_multi_u32 / BatchComparator.topk_multi on the device: every row equals the ranking of the oracle's per-candidate scores -- None dropped,
ordered by (score, index), the first k -- and equals topk() of the same comparator, over the smallest corpora that reach every branch of the
fused kernel (a last tile with padding slots, ragged lengths with exact and mixed tiles and empty candidates, `char` symbols), with copies and
near-copies of every query planted across tiles so that the index tie-break decides, for lists that form groups of 4, 2 and 1, both ops, no /
loose / tight cutoffs, k up to 65 and beyond n.  Which road a list took is read from RF_TRACE_PLAN in child processes (tests/topk_multi_check.py)."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE32, U64MAX = np.uint32(0xFFFFFFFF), np.uint64(0xFFFFFFFFFFFFFFFF)
GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel, "lcs_seq": rf.distance.lcs_seq, "osa": rf.distance.osa,
       "damerau_levenshtein": rf.distance.damerau_levenshtein}
ORA = {"levenshtein": o.levenshtein, "indel": o.indel, "lcs_seq": o.lcs_seq, "osa": o.osa}
QLEN = {"64": 64, "64b": 64, "33": 33, "33b": 33, "32": 32, "32b": 32, "20": 20, "20b": 20, "1": 1}
# lists of 1, 2, 3, 4, 5 and 7 queries: groups of 4, 2 and 1 all occur, and the last one mixes lengths <= 32 and > 32, which splits its groups
LISTS = {1: ["64"], 2: ["64", "64b"], 3: ["20", "32", "1"], 4: ["64", "64b", "33", "33b"], 5: ["20", "32", "1", "20b", "32b"],
         7: ["64", "20", "33", "32", "1", "64b", "20b"]}
GREEK_CYRILLIC = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()] + [chr(c) for c in range(0x410, 0x450)]


class Case:
    """One corpus with its planted rows: the device corpus, the comparators, and the oracle's scores (computed once per question, never changed)."""

    def __init__(self, kind):
        rng = np.random.default_rng({"a": 1, "b": 2, "c": 3, "d": 4}[kind])
        self.kind = kind
        wide = kind == "d"
        alphabet = GREEK_CYRILLIC if wide else [bytes([c]) for c in range(48, 122)]
        edit = "€" if wide else b"~"  # a symbol no query and no random candidate holds: every edit costs exactly one
        join = "".join if wide else b"".join
        rand = lambda ln: join(alphabet[i] for i in rng.integers(0, len(alphabet), size=ln))  # noqa: E731
        self.queries = {name: rand(ln) for name, ln in QLEN.items()}
        if kind == "a":    # single length 64, an odd number of tiles, the last one with padding slots beyond n
            lens = [64] * (64 * 9 - 27)
        elif kind == "b":  # single length 20
            lens = [20] * (64 * 5 + 11)
        elif kind == "c":  # ragged 0..64: lengths with whole exact tiles (20, 33, 64), everything else in mixed tiles, empty candidates
            lens = [int(x) for x in np.where(rng.random(3001) < 0.4, rng.choice([20, 33, 64], size=3001), rng.integers(0, 65, size=3001))]
            lens[5] = lens[700] = lens[2999] = 0
        else:              # `char` candidates, ragged
            lens = [int(x) for x in rng.integers(0, 65, size=64 * 10 + 5)]
        fixed = kind in "ab"
        cands = [rand(ln) for ln in lens]
        n = len(cands)
        # planted rows: per query 2 copies and rows at 1, 2 and 3 edits, walked through the corpus with a stride that is no multiple of a tile: equal
        # scores land in different tiles and different wavefronts' ranges.  The queries of 64 and 20 symbols get 20 rows at one edit: more than
        # 16 rows tied at the 16th score.
        at, stride = 3, 37
        for name, q in self.queries.items():
            for edits, rows in ((0, 2), (1, 20 if name in ("64", "20") else 4), (2, 3), (3, 3)):
                for r in range(rows):
                    row = list(q) if wide else [bytes([c]) for c in q]
                    if fixed:  # cut or repeated to the corpus' length
                        row = [row[i % len(row)] for i in range(lens[0])]
                    for pos in rng.choice(len(row), size=min(edits, len(row)), replace=False):
                        row[int(pos)] = edit
                    cands[at % n] = join(row)
                    at += stride
        self.cands, self.n = cands, n
        self.corpus = rf.Corpus.from_list(cands)
        if wide:  # the oracle sees the same strings through an injective char -> byte map
            syms = sorted({ch for s in cands + list(self.queries.values()) for ch in s})
            assert len(syms) <= 256
            table = {ch: i for i, ch in enumerate(syms)}
            self.ren = lambda s: bytes(table[ch] for ch in s)
        else:
            self.ren = lambda s: s
        self.data, self.offsets = rf.ragged([self.ren(c) for c in cands])
        self._bc = {}

    def bc(self, metric, name):
        key = (metric, name)
        if key not in self._bc:
            self._bc[key] = GPU[metric].BatchComparator(self.queries[name])
        return self._bc[key]

    @functools.lru_cache(maxsize=None)
    def scores(self, metric, name, op, cutoff=None, weights=None):
        """the oracle's per-candidate values as uint32, None = 0xFFFFFFFF (damerau_levenshtein: tests/dl_reference.py, the repository's reference for it)"""
        q = self.ren(self.queries[name])
        if metric == "damerau_levenshtein":
            if not hasattr(self, "_rows"):
                self._rows = R.ragged_rows(self.data, self.offsets)
            return R.ops(op, q, self._rows[0], self._rows[1], cutoff)
        kw = {}
        if cutoff is not None:
            kw["score_cutoff"] = cutoff
        if weights is not None and metric == "levenshtein":
            kw["weights"] = weights
        exp = ORA[metric].BatchComparator(q).many(op, self.data, self.offsets, nthreads=8, **kw)
        return np.where(exp == U64MAX, NONE32, exp.astype(np.uint32))

    def expected(self, metric, name, op, k, cutoff=None, weights=None, base=0):
        s = self.scores(metric, name, op, cutoff, weights)
        idx = np.nonzero(s != NONE32)[0]
        v = s[idx].astype(np.int64)
        order = np.lexsort((idx, -v if op == N.OP_SIMILARITY else v))[:k]
        return s[idx][order], (idx[order] + base).astype(np.uint64)

    @functools.lru_cache(maxsize=None)
    def single(self, metric, name, op, k, cutoff=None, weights=None, base=0):
        return self.bc(metric, name).topk(self.corpus, k, op, index_base=base, score_cutoff=cutoff, weights=weights)


@functools.lru_cache(maxsize=None)
def case(kind):
    return Case(kind)


def check_list(c, members, k, op, cutoff=None, weights=None, base=0):
    """members: (metric, query name) pairs.  Every row against the oracle's ranking and against topk() of the same comparator."""
    got = GPU[members[0][0]].BatchComparator.topk_multi([c.bc(m, name) for m, name in members], c.corpus, k, op, index_base=base, score_cutoff=cutoff,
                                                        weights=weights)
    assert len(got) == len(members)
    for (metric, name), (s, i) in zip(members, got):
        what = (c.kind, metric, name, k, op, cutoff, weights)
        es, ei = c.expected(metric, name, op, k, cutoff, weights, base)
        assert s.dtype == np.uint32 and i.dtype == np.uint64
        assert s.tolist() == es.tolist() and i.tolist() == ei.tolist(), what
        ss, si = c.single(metric, name, op, k, cutoff, weights, base)
        assert s.tolist() == ss.tolist() and i.tolist() == si.tolist(), what
    return got


@pytest.mark.parametrize("k", [1, 16, 64, 65])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_rows_equal_the_oracle_ranking_and_topk(kind, k):
    c = case(kind)
    for names in LISTS.values():
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
            check_list(c, [("levenshtein", name) for name in names], k, op)


def test_the_index_tie_break_decides():
    """the planted rows do what they are for: in corpus (a) more rows are tied at the 16th score than the first 16 hold of them, and the copies tie at k = 1"""
    c = case("a")
    for name in ("64", "20"):
        s = c.scores("levenshtein", name, N.OP_DISTANCE)
        es, _ = c.expected("levenshtein", name, N.OP_DISTANCE, 16)
        assert int((s == es[-1]).sum()) > int((es == es[-1]).sum()) >= 1, name
    s = c.scores("levenshtein", "64", N.OP_DISTANCE)
    assert int((s == s.min()).sum()) >= 2


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("metric", ["indel", "lcs_seq"])
def test_lcs_family_groups(kind, metric):
    c = case(kind)
    for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        check_list(c, [(metric, name) for name in LISTS[7]], 16, op)
        check_list(c, [(metric, name) for name in LISTS[4]], 64, op)


@pytest.mark.parametrize("kind", ["a", "c", "d"])
@pytest.mark.parametrize("weights", [None, (1, 2, 3), (2, 2, 5)])
def test_mixed_metrics(kind, weights):
    """one list over every usize metric: levenshtein, indel and lcs_seq pair up within their families, osa and damerau_levenshtein go per query;
    under a general weight table (1, 2, 3) the levenshtein queries go per query as well, under (2, 2, 5) they run as Indel x 2"""
    c = case(kind)
    members = [("levenshtein", "64"), ("indel", "64"), ("lcs_seq", "20"), ("osa", "64"), ("damerau_levenshtein", "20"), ("levenshtein", "64b"),
               ("indel", "33"), ("lcs_seq", "32"), ("osa", "20"), ("levenshtein", "20"), ("levenshtein", "1")]
    for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        check_list(c, members, 16, op, weights=weights)


@pytest.mark.parametrize("kind", ["a", "c"])
def test_cutoffs(kind):
    """a loose cutoff (the fused kernel; few rows pass, so count < k) and a tight one (3: the per-query early-out road)"""
    c = case(kind)
    lev = [("levenshtein", name) for name in LISTS[7]]
    for k in (16, 64):
        got = check_list(c, lev, k, N.OP_DISTANCE, cutoff=48)
        if k == 64:  # only the planted rows of a 64-symbol query are within 48 edits of it
            assert all(0 < len(s) < k for (_, name), (s, _) in zip(lev, got) if QLEN[name] == 64)
        check_list(c, lev, k, N.OP_DISTANCE, cutoff=3)
        check_list(c, [("indel", name) for name in LISTS[4]], k, N.OP_DISTANCE, cutoff=100)
        check_list(c, [("indel", name) for name in LISTS[4]], k, N.OP_SIMILARITY, cutoff=30)
    got = check_list(c, lev, 64, N.OP_DISTANCE, cutoff=0)
    assert all(len(s) == 2 for (_, name), (s, _) in zip(lev, got) if QLEN[name] == 64)  # the two copies


def test_k_beyond_the_corpus_and_index_base():
    c = case("b")
    got = check_list(c, [("levenshtein", name) for name in LISTS[5]], c.n + 5, N.OP_DISTANCE)
    assert all(len(s) == c.n for s, _ in got)
    base = 2**40 + 5
    for kind in ("a", "c"):
        got = check_list(case(kind), [("levenshtein", name) for name in LISTS[7]], 16, N.OP_DISTANCE, base=base)
        assert all(int(i.min()) >= base for _, i in got)
        check_list(case(kind), [("indel", name) for name in LISTS[4]], 65, N.OP_SIMILARITY, base=base)
    # fewer candidates than k on the fused road: count = n
    tiny = rf.Corpus.from_list([b"abcd", b"abce", b"", b"xbcd", b"abcd"])
    got = rf.distance.levenshtein.BatchComparator.topk_multi([rf.distance.levenshtein.BatchComparator(q) for q in (b"abcd", b"abc")], tiny, 16)
    assert [(s.tolist(), i.tolist()) for s, i in got] == [([0, 0, 1, 1, 4], [0, 4, 1, 3, 2]), ([1, 1, 1, 2, 3], [0, 1, 4, 3, 2])]


def test_errors_and_empty_inputs_on_the_device():
    c = case("b")
    lev = rf.distance.levenshtein.BatchComparator
    assert lev.topk_multi([], c.corpus, 4) == []
    with pytest.raises(rf.RfError) as e:
        lev.topk_multi([c.bc("levenshtein", "20")], c.corpus, 0)
    assert e.value.status == N.RF_ERR_INVALID_ARG
    with pytest.raises(rf.RfError) as e:
        lev.topk_multi([c.bc("levenshtein", "20"), rf.distance.jaro.BatchComparator(b"abc")], c.corpus, 4)
    assert e.value.status == N.RF_ERR_INVALID_ARG
    empty = rf.Corpus.from_list([])
    got = lev.topk_multi([c.bc("levenshtein", "20"), c.bc("levenshtein", "20b")], empty, 4)
    assert [len(s) for s, _ in got] == [0, 0]


@pytest.mark.parametrize("missing", ["out_score", "out_index"])
def test_a_null_row_array_over_a_non_empty_corpus_writes_nothing(missing):
    import ctypes as C

    c = case("b")
    cs = [c.bc("levenshtein", "20"), c.bc("levenshtein", "20b")]
    hs = (C.c_void_p * 2)(*[x._h for x in cs])
    args = rf.Args().to_c(False)
    score, index, count = np.full((2, 4), 77, dtype=np.uint32), np.full((2, 4), 77, dtype=np.uint64), np.full(2, 77, dtype=np.uint32)
    st = N.lib().rf_topk_multi_u32(hs, 2, c.corpus._h, N.OP_DISTANCE, C.byref(args), 4, 0, None if missing == "out_score" else score.ctypes.data,
                                   None if missing == "out_index" else index.ctypes.data, count.ctypes.data, None)
    assert st == N.RF_ERR_INVALID_ARG
    assert (count == 77).all() and (score == 77).all() and (index == 77).all()


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "topk_multi_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_roads_by_the_plan_trace():
    """a child process with RF_TRACE_PLAN: a loose-cutoff list runs fused, the tight-cutoff list and the k = 65 list go per query, and with
    RF_TOPK_MULTI=0 every list does -- with the same rows"""
    r = _child("roads")
    assert "roads ok" in r.stdout, r.stdout[-2000:]
    r = _child("roads_off", RF_TOPK_MULTI="0")
    assert "roads_off ok" in r.stdout, r.stdout[-2000:]


def test_several_tiles_per_wavefront():
    """tests/topk_multi_check.py with one workgroup per CU and a sample of 8 tiles: every wavefront of the fused kernel owns at least 3 tiles, the
    last a partial one; single-length and ragged corpora, 64-bit and 32-bit Levenshtein and Indel, q = 4, k = 16, every row against the oracle's
    ranking; the checker asserts from the plan lines that groups of 4 ran fused and that the sample pass ran"""
    r = _child("multitile", RF_SCAN_BLOCKS_PER_CU="1", RF_TOPK_SAMPLE="8")
    assert "FAILURES 0" in r.stdout, r.stdout[-3000:]
