"""Run by tests/test_gpu_layouts_multi.py, one child process per leg, with the leg's pack-time knobs and RF_TRACE_PLAN=1 in the environment (the library reads
its switches once per process):

  layout_multi_check.py save <P file> <QC file>                          pack the two corpora of tests/layout_multi_inputs.py under this process' knobs, save them
  layout_multi_check.py <leg> <no_mixed: 0 | 1> [<P file> <QC file>]     the multi-query and join roads over the corpora packed here -- or loaded from the two files --
                                                                         against the CPU oracle

Sections (each reports its own failures; a HIP error ends the process at once):
  layout        slot_index() of P and QC: a permutation of the candidates padded with kPad, the pads where the counts say under RF_NO_MIXED_TILES
                (test_gpu_layouts._check_layout)
  filter_u32    filter_multi of all eleven queries, levenshtein / indel / lcs_seq x distance / similarity x both tight cutoffs of join_check.CUTOFFS, every order,
                and a capacity below the counts; a loose cutoff and osa on the per-query road
  filter_f64    levenshtein / indel by normalized score, the ratio, jaro_winkler (per query)
  topk_u32/f64  topk_multi, k in {1, 16, 64} and -- u32 -- n + 5
  join_u32      QC x P (by query, any order, capacity 0 and below the count, query_indices), P x QC, QC x QC with and without upper
  join_f64      QC x P
  cross         file legs only: the loaded corpus on one side of a join, the same data packed here without a knob on the other

The road every tight-cutoff call took is read from its "[rf plan]" lines.  The planner's rules give, on every layout:
  filter_multi  a query is fused when plan() sets `early` (the cutoffs are tight for every length) and it has <= 64 symbols; group_queries() collects, from the first
                untaken query forward, up to 4 of one class (<= 32 symbols / 33..64).  Q's lengths 0, 1, 5, 20, 20, 32 | 33, 33, 64, 64 | 65 give the groups
                [4, 2, 4] -- in the order of their first members -- and the 65-symbol query per query
  join          every row of <= 64 symbols fused: one batch, ceil(narrow / 4) + ceil(wide / 4) items (join_check.expected_groups), the longer rows per query
Exit status 0 and "FAILURES 0" = all as expected."""
import os
import sys
import time
import traceback
from types import SimpleNamespace

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]

import layout_multi_inputs as I  # noqa: E402
import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402

J, F = I.J, I.F
ORDERS = (N.FILTER_BY_INDEX, N.FILTER_BY_SCORE, N.FILTER_ANY)
FUSED = {"q": 11, "groups": [4, 2, 4], "per_query": 1}
PER_QUERY = {"q": 11, "groups": [], "per_query": 11}


class Plan(J.PlanLines):
    """the "[rf plan] <road>:" lines the library wrote to stderr inside the block"""

    def __init__(self, road):
        self.road = road

    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.lines = [ln for ln in self.text.splitlines() if ln.startswith(f"[rf plan] {self.road}:")]
        return False


def gpu_class(is_f, metric):
    return F.gpu_class(metric) if is_f else J.GPU[metric].BatchComparator


_comparators = {}


def comparators(cls):
    if cls not in _comparators:
        _comparators[cls] = [cls(q) for q in I.queries()]
    return _comparators[cls]


def pairs(is_f, i, s):
    return list(zip(np.asarray(i).tolist(), I.score_list(is_f, s)))


# ---- a. the layout
def check_layout(corpus, c, no_mixed, loaded):
    import test_gpu_layouts as L

    assert len(corpus) == c.n
    si = corpus.slot_index()
    assert len(si) == corpus.slot_count and corpus.slot_count % 64 == 0
    real = si != I.NONE32
    assert int((~real).sum()) == corpus.slot_count - c.n
    assert np.array_equal(np.sort(si[real]), np.arange(c.n, dtype=np.uint32))
    L._check_layout(SimpleNamespace(corpus=corpus, shape="bytes", data=c.data, offsets=c.offsets), c.counts, no_mixed, si, loaded)
    pad, tile_len = I.pad_map(c.counts)
    if no_mixed:
        assert np.array_equal(si == I.NONE32, pad)
        t = int(np.nonzero(tile_len == 33)[0][-1])
        assert int(real[64 * t: 64 * t + 64].sum()) == 1  # the tile with one live lane
    else:
        assert len(si) != len(pad) or not np.array_equal(si == I.NONE32, pad)


# ---- b / c. filter_multi
def check_filter(P, is_f, metric, op, cutoff, want):
    from filter_multi_check import parse  # (the line has one form for rf_filter_multi_u32 and rf_filter_multi_f64)

    cls = gpu_class(is_f, metric)
    cs = comparators(cls)
    what = (metric, op, cutoff)
    for order in ORDERS:
        with Plan("filter_multi_f64" if is_f else "filter_multi") as pl:
            got = cls.filter_multi(cs, op, P, order=order, score_cutoff=cutoff)
        counts = list(cls.last_filter_counts)
        road = [parse(ln) for ln in pl.lines]
        assert road and all(r == want for r in road), (what, order, pl.lines, want)
        for j, q in enumerate(I.queries()):
            i, s = got[j]
            assert i.dtype == np.uint64 and s.dtype == (np.float64 if is_f else np.uint32)
            ei, es = I.ranked(is_f, metric, op, cutoff, q) if order == N.FILTER_BY_SCORE else I.somes(is_f, metric, op, cutoff, q)
            assert counts[j] == len(ei), (what, order, j, counts[j], len(ei))
            g, e = pairs(is_f, i, s), pairs(is_f, ei, es)
            assert (sorted(g) if order == N.FILTER_ANY else g) == e, (what, order, j, g[:4], e[:4])
    # a capacity below the counts: the count is the true one, the row holds `capacity` distinct matches in the requested order among themselves
    cap = 3
    for order in ORDERS:
        got = cls.filter_multi(cs, op, P, capacity=cap, order=order, score_cutoff=cutoff)
        counts = list(cls.last_filter_counts)
        over = 0
        for j, q in enumerate(I.queries()):
            i, s = got[j]
            ei, es = I.somes(is_f, metric, op, cutoff, q)
            assert counts[j] == len(ei) and len(i) == len(s) == min(len(ei), cap), (what, order, j, counts[j], len(ei), len(i))
            assert len(set(i.tolist())) == len(i)
            known = dict(pairs(is_f, ei, es))
            assert all(known.get(a) == b for a, b in pairs(is_f, i, s)), (what, order, j)
            if order == N.FILTER_BY_INDEX:
                assert i.tolist() == sorted(i.tolist())
            elif order == N.FILTER_BY_SCORE:
                v = s.astype(np.float64)
                key = list(zip((-v if I.descending(op) else v).tolist(), i.tolist()))
                assert key == sorted(key), (what, j)
            over += len(ei) > cap
        assert over > 0, what


# ---- d / e. topk_multi
def check_topk(P, n, is_f, metric, op, cutoff, ks):
    cls = gpu_class(is_f, metric)
    cs = comparators(cls)
    for k in ks:
        got = cls.topk_multi(cs, P, k, op, score_cutoff=cutoff)
        for j, q in enumerate(I.queries()):
            s, i = got[j]
            ei, es = I.ranked(is_f, metric, op, cutoff, q)
            m = min(k, len(ei))
            what = (metric, op, cutoff, k, j)
            assert len(i) == len(s) == m, (what, len(i), m)
            if cutoff is None:
                assert len(ei) == n and m == min(k, n)  # without a cutoff every candidate has a score: k = n + 5 returns exactly n entries
            assert (i < n).all() and len(set(i.tolist())) == len(i), what  # every index a candidate's, each once: no padding lane, none twice
            assert pairs(is_f, i, s) == pairs(is_f, ei[:m], es[:m]), (what, pairs(is_f, i, s)[:4], pairs(is_f, ei[:m], es[:m])[:4])


# ---- f / g. joins
def join(is_f, metric, queries, corpus, op, cutoff, **kw):
    if is_f:
        return F.got_triples(F.join(metric, queries, corpus, op, cutoff, **kw))
    return J.got_triples(J.GPU[metric].BatchComparator.join(queries, corpus, op, score_cutoff=cutoff, **kw))


def oracle(is_f, which, metric, op, cutoff):
    return (I.oracle_f64 if is_f else I.oracle_u32)(which, metric, op, cutoff)


def join_plan(is_f, lens):
    """what the plan line must say for rows of these lengths"""
    batches, groups = J.expected_groups([x for x in lens if x <= 64], 16384)
    return {"m": len(lens), "batches": batches, "groups": groups, "per_query": sum(1 for x in lens if x > 64)}


def planned_join(is_f, metric, queries, corpus, op, cutoff, lens, **kw):
    with Plan("join_f64" if is_f else "join") as pl:
        got = join(is_f, metric, queries, corpus, op, cutoff, **kw)
    road = [(F.parse if is_f else J.parse)(ln) for ln in pl.lines]
    want = join_plan(is_f, lens)
    assert road and all(r == want for r in road), ((metric, op, cutoff), pl.lines, want)
    return got


def check_join(P, QC, is_f, metric, op, cutoff, with_indices):
    qc = I.query_corpus()
    cls = gpu_class(is_f, metric)
    what = (metric, op, cutoff)
    ora = oracle(is_f, "P", metric, op, cutoff)
    exp = ora.triples(qc.rows)
    lens = [len(r) for r in qc.rows]
    assert len(exp) > len(I.queries())
    got = planned_join(is_f, metric, QC, P, op, cutoff, lens)
    assert got == exp, (what, len(got), len(exp), [t for t in got if t not in set(exp)][:4], [t for t in exp if t not in set(got)][:4])
    assert sorted(join(is_f, metric, QC, P, op, cutoff, order=N.JOIN_ANY)) == exp, what
    # capacity 0: the count only; a capacity below the count: that many distinct triples of the answer, in order
    assert join(is_f, metric, QC, P, op, cutoff, capacity=0) == [] and cls.last_join_count == len(exp), (what, cls.last_join_count, len(exp))
    cap = len(exp) // 2
    for order in (N.JOIN_BY_QUERY, N.JOIN_ANY):
        part = join(is_f, metric, QC, P, op, cutoff, capacity=cap, order=order)
        assert cls.last_join_count == len(exp) and len(part) == cap and len(set(part)) == cap and set(part) <= set(exp), (what, order, len(part), cls.last_join_count)
        if order == N.JOIN_BY_QUERY:
            assert part == sorted(part)
    if with_indices:
        qi = I.join_query_indices()
        got = planned_join(is_f, metric, QC, P, op, cutoff, [lens[r] for r in qi], query_indices=qi)
        assert got == ora.triples(qc.rows, qi), (what, "query_indices")


def check_join_swapped_and_self(P, QC):
    """P x QC: the small corpus is scanned, so nearly every window is empty or a single tile; QC x QC with and without upper"""
    p, qc = I.scanned(), I.query_corpus()
    ora = I.oracle_u32("QC", "levenshtein", I.DIST, 3)
    exp = ora.triples(p.cands)
    got = planned_join(False, "levenshtein", P, QC, I.DIST, 3, [len(c) for c in p.cands])
    assert len(exp) > 100 and got == exp, (len(got), len(exp))
    lens = [len(r) for r in qc.rows]
    full = planned_join(False, "levenshtein", QC, QC, I.DIST, 3, lens)
    assert full == ora.triples(qc.rows) and all((i, i, 0) in set(full) for i in range(qc.n))
    upper = planned_join(False, "levenshtein", QC, QC, I.DIST, 3, lens, upper=True)
    assert upper == ora.triples(qc.rows, upper=True) == [t for t in full if t[0] < t[1]] and len(upper) > 0


# ---- h. the two sides of a join in different layouts
def check_cross(P, QC):
    p, qc = I.scanned(), I.query_corpus()
    P2, QC2 = rf.Corpus.from_ragged(p.data, p.offsets), rf.Corpus.from_ragged(qc.data, qc.offsets)  # (this process has no pack-time knob set)
    assert not any(os.environ.get(k) for k in ("RF_NO_MIXED_TILES", "RF_NO_RENAME"))
    qlens, plens = [len(r) for r in qc.rows], [len(c) for c in p.cands]
    for is_f, metric, op, cutoff in ((False, "levenshtein", I.DIST, 3), (True, "ratio", I.SIM, 0.9)):
        exp = oracle(is_f, "P", metric, op, cutoff).triples(qc.rows)
        for a, b in ((QC, P2), (QC2, P)):
            got = planned_join(is_f, metric, a, b, op, cutoff, qlens)
            assert got == exp, (metric, "loaded queries" if a is QC else "loaded corpus", len(got), len(exp))
    exp = I.oracle_u32("QC", "levenshtein", I.DIST, 3).triples(p.cands)
    for a, b in ((P, QC2), (P2, QC)):
        got = planned_join(False, "levenshtein", a, b, I.DIST, 3, plens)
        assert got == exp, ("swapped", "loaded queries" if a is P else "loaded corpus", len(got), len(exp))


def save(p_path, qc_path):
    p, qc = I.scanned(), I.query_corpus()
    for c, path in ((p, p_path), (qc, qc_path)):
        lay = rf.host_layout(c.data, c.offsets)  # (follows this process' knobs, as the packers do)
        assert (lay["n_mixed"] == 0) == bool(os.environ.get("RF_NO_MIXED_TILES"))
        assert np.array_equal(lay["sigma"], np.arange(256, dtype=np.uint8)) == bool(os.environ.get("RF_NO_RENAME"))
        rf.Corpus.from_ragged(c.data, c.offsets).save(path)
    return 0


def roads(leg, no_mixed, files):
    p, qc = I.scanned(), I.query_corpus()
    if files:
        P, QC = rf.Corpus.load(files[0]), rf.Corpus.load(files[1])
    else:
        P, QC = rf.Corpus.from_ragged(p.data, p.offsets), rf.Corpus.from_ragged(qc.data, qc.offsets)
        if leg == "no_rename":
            assert np.array_equal(rf.host_layout(p.data, p.offsets)["sigma"], np.arange(256, dtype=np.uint8))
    failures = []

    def section(name, fn, *args):
        t0 = time.perf_counter()
        try:
            fn(*args)
            verdict = "ok"
        except AssertionError:
            failures.append(name)
            verdict = "FAILED\n" + traceback.format_exc(limit=4)[-3000:]
        print(f"[{leg}] {name}: {verdict} ({time.perf_counter() - t0:.2f} s)", flush=True)

    section("layout P", check_layout, P, p, no_mixed, bool(files))
    section("layout QC", check_layout, QC, qc, no_mixed, bool(files))
    for metric, op, cutoff in I.U32_FILTER:
        section(f"filter_u32 {metric} op {op} cutoff {cutoff}", check_filter, P, False, metric, op, cutoff, FUSED)
    for metric, op, cutoff in I.U32_PER_QUERY:
        section(f"filter_u32 {metric} op {op} cutoff {cutoff} (per query)", check_filter, P, False, metric, op, cutoff, PER_QUERY)
    for metric, op, cutoff in I.F64_FILTER:
        section(f"filter_f64 {metric} op {op} cutoff {cutoff}", check_filter, P, True, metric, op, cutoff, FUSED)
    for metric, op, cutoff in I.F64_PER_QUERY:
        section(f"filter_f64 {metric} op {op} cutoff {cutoff} (per query)", check_filter, P, True, metric, op, cutoff, PER_QUERY)
    for metric, op, cutoff in I.U32_TOPK:
        section(f"topk_u32 {metric} op {op} cutoff {cutoff}", check_topk, P, p.n, False, metric, op, cutoff, (1, 16, 64, p.n + 5))
    for metric, op, cutoff in I.F64_TOPK:
        section(f"topk_f64 {metric} op {op}", check_topk, P, p.n, True, metric, op, cutoff, (1, 16, 64))
    for metric, op, cutoff in I.U32_JOIN:
        section(f"join_u32 {metric} op {op} cutoff {cutoff}", check_join, P, QC, False, metric, op, cutoff, True)
    section("join_u32 P x QC, QC x QC", check_join_swapped_and_self, P, QC)
    for metric, op, cutoff in I.F64_JOIN:
        section(f"join_f64 {metric} op {op} cutoff {cutoff}", check_join, P, QC, True, metric, op, cutoff, False)
    if files:
        section("cross-layout joins", check_cross, P, QC)
    print("FAILED SECTIONS", failures)
    print("FAILURES", len(failures))
    return len(failures)


if __name__ == "__main__":
    if sys.argv[1] == "save":
        sys.exit(save(sys.argv[2], sys.argv[3]))
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    sys.exit(1 if roads(sys.argv[1], sys.argv[2] == "1", sys.argv[3:5]) else 0)
