"""rf_filter_multi_u32 / BatchComparator.filter_multi on the device: every row equals the oracle's per-candidate values with the Nones dropped -- in the
order asked for -- and equals filter_many() of the same comparator, over the smallest corpora that reach every branch of the fused kernel (a last tile
with padding slots, ragged lengths with exact and mixed tiles and empty candidates, `char` symbols), with copies, near-copies and prefix sharers of every
query planted across tiles (rows that survive the looks at columns 8 and 16 and die later), for lists that form groups of 4, 2 and 1, both ops, tight /
loose / no cutoffs, capacities below the counts and a pure count.  Which road a list took is read from RF_TRACE_PLAN in child processes
(tests/filter_multi_check.py)."""
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
ORDERS = (N.FILTER_BY_INDEX, N.FILTER_BY_SCORE, N.FILTER_ANY)
GREEK_CYRILLIC = [chr(c) for c in range(0x391, 0x3CA) if chr(c).isalpha()] + [chr(c) for c in range(0x410, 0x450)]


class Case:
    """One corpus with its planted rows: the device corpus, the comparators, and the oracle's scores (computed once per question, never changed)."""

    def __init__(self, kind):
        rng = np.random.default_rng({"a": 11, "b": 12, "c": 13, "d": 14}[kind])
        self.kind = kind
        wide = kind == "d"
        alphabet = GREEK_CYRILLIC if wide else [bytes([c]) for c in range(48, 122)]
        edit = "€" if wide else b"~"  # a symbol no query and no random candidate holds: every edit costs exactly one
        join = "".join if wide else b"".join
        rand_syms = lambda ln: [alphabet[i] for i in rng.integers(0, len(alphabet), size=ln)]  # noqa: E731
        rand = lambda ln: join(rand_syms(ln))  # noqa: E731
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
        self.max_len = max(lens)
        cands = [rand(ln) for ln in lens]
        n = len(cands)
        # planted rows, walked through the corpus with a stride that is no multiple of a tile (37 shares no factor with any n here, and there are fewer
        # planted rows than candidates: none overwrites another): per query 2 copies, rows at 1, 2 and 3 edits -- 20 at one edit for two of the queries --
        # and 6 prefix sharers: the query's first 24 symbols (12 for the queries of <= 20), random behind them
        at, stride = 3, 37
        planted = []
        for name, q in self.queries.items():
            syms = list(q) if wide else [bytes([c]) for c in q]
            shape = lambda row: [row[i % len(row)] for i in range(lens[0])] if fixed else list(row)  # noqa: E731  (cut or repeated to the corpus' length)
            for edits, rows in ((0, 2), (1, 20 if name in ("64", "20") else 4), (2, 3), (3, 3)):
                for r in range(rows):
                    row = shape(syms)
                    for pos in rng.choice(len(row), size=min(edits, len(row)), replace=False):
                        row[int(pos)] = edit
                    planted.append(row)
            keep = min(len(syms), 12 if len(syms) <= 20 else 24)
            for r in range(6):
                row = shape(syms)
                row[min(keep, len(row)):] = rand_syms(max(len(row) - keep, 0))  # (a single-length corpus shorter than the prefix: a copy)
                planted.append(row)
        assert len(planted) < n
        for row in planted:
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
        if metric == "levenshtein" and op == N.OP_SIMILARITY and cutoff is not None:
            # Q2: above its cutoff the reference's Levenshtein similarity is a wrapped value where the device returns None.  The expectation is the
            # oracle's own un-cut similarity, kept where it reaches the cutoff -- and there the oracle's value under the cutoff must be that very value
            kw.pop("score_cutoff")
            full = ORA[metric].BatchComparator(q).many(op, self.data, self.offsets, nthreads=8, **kw)
            keep = full >= np.uint64(cutoff)
            assert (exp[keep] == full[keep]).all()
            exp = np.where(keep, full, U64MAX)
        return np.where(exp == U64MAX, NONE32, exp.astype(np.uint32))

    def expected(self, metric, name, op, order, cutoff=None, weights=None, base=0):
        """(indices, scores) of the oracle's Somes: ascending index, or best score first with ties by index"""
        s = self.scores(metric, name, op, cutoff, weights)
        idx = np.nonzero(s != NONE32)[0]
        if order == N.FILTER_BY_SCORE:
            v = s[idx].astype(np.int64)
            idx = idx[np.lexsort((idx, -v if op == N.OP_SIMILARITY else v))]
        return (idx + base).astype(np.uint64), s[idx]

    @functools.lru_cache(maxsize=None)
    def single(self, metric, name, op, order, cutoff=None, weights=None, base=0):
        return self.bc(metric, name).filter_many(op, self.corpus, order=order, index_base=base, score_cutoff=cutoff, weights=weights)


@functools.lru_cache(maxsize=None)
def case(kind):
    return Case(kind)


def pairs(i, s):
    return sorted(zip(i.tolist(), s.tolist()))


def check_list(c, members, op, cutoff=None, weights=None, base=0, orders=ORDERS):
    """members: (metric, query name) pairs.  Every row against the oracle's Somes and against filter_many() of the same comparator, capacity ample."""
    got = None
    for order in orders:
        got = GPU[members[0][0]].BatchComparator.filter_multi([c.bc(m, name) for m, name in members], op, c.corpus, order=order, index_base=base,
                                                              score_cutoff=cutoff, weights=weights)
        assert len(got) == len(members)
        for (metric, name), (i, s) in zip(members, got):
            what = (c.kind, metric, name, op, cutoff, weights, order)
            ei, es = c.expected(metric, name, op, order, cutoff, weights, base)
            si, ss = c.single(metric, name, op, order, cutoff, weights, base)
            assert i.dtype == np.uint64 and s.dtype == np.uint32
            if order == N.FILTER_ANY:
                assert pairs(i, s) == pairs(ei, es) == pairs(si, ss), what
            else:
                assert i.tolist() == ei.tolist() and s.tolist() == es.tolist(), what
                assert i.tolist() == si.tolist() and s.tolist() == ss.tolist(), what
    return got


@pytest.mark.parametrize("cutoff", [0, 1, 3, 5, 48, None])
@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_levenshtein_rows_equal_the_oracle_and_filter_many(kind, cutoff):
    """cutoffs 0, 1, 3 and 5 run fused, 48 (loose) and no cutoff go per query"""
    c = case(kind)
    for names in LISTS.values():
        check_list(c, [("levenshtein", name) for name in names], N.OP_DISTANCE, cutoff)


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
def test_levenshtein_similarity_rows(kind):
    """similarity >= len - 3, len = the corpus' longest candidate: a tight cutoff for the queries about that long"""
    c = case(kind)
    for names in LISTS.values():
        check_list(c, [("levenshtein", name) for name in names], N.OP_SIMILARITY, c.max_len - 3)


def test_the_planted_rows_do_what_they_are_for():
    """corpus (a): the 64-symbol query has its 2 copies + 20 rows at one edit within cutoff 1, and its prefix sharers are beyond every cutoff used
    here although their first 24 symbols are the query's: they survive the looks at columns 8 and 16 under cutoffs 3 and 5"""
    c = case("a")
    s = c.scores("levenshtein", "64", N.OP_DISTANCE)
    assert int((s <= 1).sum()) == 22 and int((s == 0).sum()) == 2
    q = c.queries["64"]
    sharers = [i for i, cand in enumerate(c.cands) if cand[:24] == q[:24] and s[i] > 5]
    assert len(sharers) == 6
    for i in sharers:  # the distance of the 16-symbol prefixes is 0: the bound after the first chunk cannot exceed any cutoff
        assert c.cands[i][:16] == q[:16]


@pytest.mark.parametrize("kind", ["a", "b", "c", "d"])
@pytest.mark.parametrize("metric", ["indel", "lcs_seq"])
def test_lcs_family_groups(kind, metric):
    """distance cutoff 6, and a similarity cutoff close enough to the maximum for plan() to set `early` for the queries about as long as the corpus'
    longest candidate: 2 len - 8 for indel (maximum len1 + len2), len - 4 for lcs_seq (maximum max(len1, len2))"""
    c = case(kind)
    sim = 2 * c.max_len - 8 if metric == "indel" else c.max_len - 4
    for n in (4, 7):
        members = [(metric, name) for name in LISTS[n]]
        check_list(c, members, N.OP_DISTANCE, 6, orders=ORDERS[:2])
        check_list(c, members, N.OP_SIMILARITY, sim, orders=ORDERS[:2])


@pytest.mark.parametrize("kind", ["a", "c", "d"])
@pytest.mark.parametrize("weights", [None, (1, 2, 3), (2, 2, 5)])
def test_mixed_metrics(kind, weights):
    """one list over every usize metric under cutoff 6: levenshtein, indel and lcs_seq pair up within their families, osa and damerau_levenshtein go per
    query; under a general weight table (1, 2, 3) the levenshtein queries go per query as well, under (2, 2, 5) they run as Indel x 2"""
    c = case(kind)
    members = [("levenshtein", "64"), ("indel", "64"), ("lcs_seq", "20"), ("osa", "64"), ("damerau_levenshtein", "20"), ("levenshtein", "64b"),
               ("indel", "33"), ("lcs_seq", "32"), ("osa", "20"), ("levenshtein", "20"), ("levenshtein", "1")]
    check_list(c, members, N.OP_DISTANCE, 6, weights=weights, orders=ORDERS[:2])
    check_list(c, members, N.OP_SIMILARITY, c.max_len - 3, weights=weights, orders=ORDERS[:1])


@pytest.mark.parametrize("capacity", [1, 3])
def test_overflow_keeps_the_true_count_and_valid_rows(capacity):
    """cutoff 1 on corpus (a): the 64-symbol query has 22 qualifying rows.  out_count is the true count; a row's entries are distinct members of the
    expected set, in the requested order among themselves"""
    c = case("a")
    lev = rf.distance.levenshtein.BatchComparator
    for n in (4, 7):
        names = LISTS[n]
        cs = [c.bc("levenshtein", name) for name in names]
        for order in ORDERS:
            got = lev.filter_multi(cs, N.OP_DISTANCE, c.corpus, capacity=capacity, order=order, score_cutoff=1)
            counts = lev.last_filter_counts
            for name, (i, s), cnt in zip(names, got, counts):
                ei, es = c.expected("levenshtein", name, N.OP_DISTANCE, N.FILTER_BY_INDEX, 1)
                assert cnt == len(ei), (name, order)
                if name == "64":
                    assert cnt == 22
                assert len(i) == len(s) == min(cnt, capacity)
                assert len(set(i.tolist())) == len(i)
                want = dict(zip(ei.tolist(), es.tolist()))
                assert all(want.get(a) == b for a, b in zip(i.tolist(), s.tolist())), (name, order)
                if order == N.FILTER_BY_INDEX:
                    assert i.tolist() == sorted(i.tolist())
                elif order == N.FILTER_BY_SCORE:
                    assert list(zip(s.tolist(), i.tolist())) == sorted(zip(s.tolist(), i.tolist()))


def test_capacity_zero_is_a_pure_count():
    c = case("a")
    lev = rf.distance.levenshtein.BatchComparator
    for n in (4, 7):
        names = LISTS[n]
        cs = [c.bc("levenshtein", name) for name in names]
        for cutoff in (1, None):  # fused, per query
            got = lev.filter_multi(cs, N.OP_DISTANCE, c.corpus, capacity=0, score_cutoff=cutoff)  # (the wrapper passes NULL row arrays)
            assert all(len(i) == 0 and len(s) == 0 for i, s in got)
            assert lev.last_filter_counts == [len(c.expected("levenshtein", name, N.OP_DISTANCE, N.FILTER_BY_INDEX, cutoff)[0]) for name in names]


@pytest.mark.parametrize("kind", ["a", "c", "d"])
def test_index_base_beyond_32_bits(kind):
    c = case(kind)
    base = 2**40 + 5
    got = check_list(c, [("levenshtein", name) for name in LISTS[7]], N.OP_DISTANCE, 3, base=base)
    assert any(len(i) for i, _ in got) and all(int(i.min()) >= base for i, _ in got if len(i))
    check_list(c, [("indel", name) for name in LISTS[4]], N.OP_DISTANCE, 6, base=base, orders=ORDERS[:1])


def test_empty_inputs():
    c = case("b")
    lev = rf.distance.levenshtein.BatchComparator
    assert lev.filter_multi([], N.OP_DISTANCE, c.corpus, score_cutoff=3) == []
    empty = rf.Corpus.from_list([])
    got = lev.filter_multi([c.bc("levenshtein", "20"), c.bc("levenshtein", "20b")], N.OP_DISTANCE, empty, score_cutoff=3)
    assert [(len(i), len(s)) for i, s in got] == [(0, 0), (0, 0)] and lev.last_filter_counts == [0, 0]
    with pytest.raises(rf.RfError) as e:
        lev.filter_multi([c.bc("levenshtein", "20"), rf.distance.jaro.BatchComparator(b"abc")], N.OP_DISTANCE, c.corpus, score_cutoff=3)
    assert e.value.status == N.RF_ERR_INVALID_ARG


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "filter_multi_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_TRACE_PLAN="1", **env), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_roads_by_the_plan_trace():
    """a child process with RF_TRACE_PLAN: a cutoff-3 list of 7 queries shows fused groups [4,2] and 1 per query, the no-cutoff and the loose-cutoff lists
    show no fused group, and with RF_FILTER_MULTI=0 every list goes per query -- with the same rows"""
    r = _child("roads")
    assert "roads ok" in r.stdout, r.stdout[-2000:]
    r = _child("roads_off", RF_FILTER_MULTI="0")
    assert "roads_off ok" in r.stdout, r.stdout[-2000:]


def test_several_tiles_per_wavefront():
    """tests/filter_multi_check.py with one workgroup per CU: every wavefront of the fused kernel owns at least 3 tiles, the last a partial one; single-length
    and ragged corpora, 64-bit and 32-bit Levenshtein and Indel, q = 4, cutoff 3, every row against the oracle's Somes; the checker asserts from the plan
    lines that groups of 4 ran fused, and on the host that tiles with and without a planted row both occur"""
    r = _child("multitile", RF_SCAN_BLOCKS_PER_CU="1")
    assert "FAILURES 0" in r.stdout, r.stdout[-3000:]
