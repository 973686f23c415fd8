"""Run by tests/test_gpu_join_wide.py in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process): the four join calls over `char`
corpora, results AND the road each call took.

  calls       two `char` corpora -- Greek-heavy queries of 0, 1, 5, 32, 33, 64, 64 and 65 symbols, ~300 Cyrillic-heavy ragged candidates with planted near-copies,
              symbols above U+FFFF on both sides, query symbols the scanned corpus never stores, candidate symbols no query has -- through join, join_f64,
              join_topk and join_topk_f64: every result equals the CPU oracle's over a byte image of the symbols, and the plan line shows the 65-symbol row
              per query and the other seven in two groups.  With RF_JOIN=0: the same results, every row per query.  With RF_SCAN_BLOCKS_PER_CU=1: the same.
  self        one `char` handle on both sides, duplicates and near-duplicates: join with and without `upper`, join_topk with `no_self` at k = 1 and 3,
              query_indices unordered and repeated
  overflow    one handle with 254 common symbols and 46 rare ones (the overflow class): rows that hold a rare symbol go per query, the others fuse, and every
              result equals the loop of single-query filter_many / topk
  across      the overflow class on the queries' side only, on the scanned side only, on both
  mixed       byte queries against a `char` corpus; `char` queries of symbols <= 0xFF against a byte corpus; a `char` row with a symbol above 0xFF against a byte
              corpus is the per-query road's error, with the outputs untouched
  batch       RF_JOIN_BATCH=8 with 1 .. 17 rows

Expected values: the CPU oracle over a byte image of the symbols where the union of both alphabets has at most 256 symbols (the map is a bijection and every metric
here depends only on symbol equality), else the loop of single-query calls.  f64 scores are compared bit for bit.  The number of rows a call must have fused is
always computed from the inputs here, never read back from the library.  Exit status 0 = all as expected."""
import ctypes as C
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
import join_check as J  # noqa: E402
import join_f64_check as F  # noqa: E402
import join_topk_check as T  # noqa: E402
import join_topk_f64_check as TF  # noqa: E402

ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
QUERY_LENGTHS = [0, 1, 5, 32, 33, 64, 64, 65]
GREEK = [chr(c) for c in range(0x3B1, 0x3CA) if c != 0x3C2]
CYRILLIC = [chr(c) for c in range(0x430, 0x450)]
SHARED = list("abcdefgh -'")
HIGH = [chr(c) for c in (0x1F600, 0x1F601, 0x1F602, 0x10348)]  # above U+FFFF: [0], [1] on both sides, [2] candidates only, [3] queries only
QUERY_ONLY = ["ϗ", HIGH[3]]
CAND_ONLY = ["Ѣ", HIGH[2]]


class PlanLines(J.PlanLines):
    """every "[rf plan] join...:" line the library wrote to stderr inside the block, parsed: {"call", "m", "batches", "groups", "per_query"}"""

    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.road = []
        for ln in self.text.splitlines():
            m = re.match(r"\[rf plan\] (join|join_f64|join_topk|join_topk_f64): m=(\d+) (?:k=\d+ )?batches=(\d+) groups=(\d+) (?:units=\d+ )?per_query=(\d+)$", ln)
            if m:
                self.road.append({"call": m.group(1), "m": int(m.group(2)), "batches": int(m.group(3)), "groups": int(m.group(4)), "per_query": int(m.group(5))})
        return False


def want_road(call, lens, per_query, batch=16384, off=False):
    """the plan line of a call over rows of these lengths of which `per_query` -- computed by the caller from the inputs -- must not fuse; `lens` are the lengths
    of the rows that must (the groups follow tests/join_check.py's rule)"""
    if off:
        return {"call": call, "m": len(lens) + per_query, "batches": 0, "groups": 0, "per_query": len(lens) + per_query}
    batches, groups = J.expected_groups(lens, batch) if lens else (0, 0)
    return {"call": call, "m": len(lens) + per_query, "batches": batches, "groups": groups, "per_query": per_query}


class Image:
    """a bijection symbol -> byte over the union of the alphabets of some strings (at most 256 symbols), for the CPU oracle"""

    def __init__(self, *lists):
        syms = sorted({ch for rows in lists for row in rows for ch in symbols(row)})
        assert len(syms) <= 256, len(syms)
        self.of = {s: i for i, s in enumerate(syms)}

    def __call__(self, rows):
        return [bytes(self.of[ch] for ch in symbols(row)) for row in rows]


def symbols(row):
    """the code points of a str, the bytes of a bytes"""
    return [ord(ch) for ch in row] if isinstance(row, str) else list(row)


def draw(rng, alphabet, weights, n):
    w = np.asarray(weights, dtype=np.float64)
    return "".join(alphabet[int(i)] for i in rng.choice(len(alphabet), size=n, p=w / w.sum()))


def str_edits(rng, q, k, filler):
    """q after k random edits: substitutions and insertions of `filler`, deletions"""
    row = list(q)
    for _ in range(k):
        kind = int(rng.integers(0, 3))
        if kind == 0 and row:
            row[int(rng.integers(0, len(row)))] = filler
        elif kind == 1:
            row.insert(int(rng.integers(0, len(row) + 1)), filler)
        elif row:
            del row[int(rng.integers(0, len(row)))]
    return "".join(row)


def calls_case():
    """(queries, candidates): the two corpora rank their symbols differently -- the queries are mostly Greek, the candidates mostly Cyrillic, both use the shared
    ASCII and two symbols above U+FFFF; every query of 5 symbols or more holds one symbol the candidates never have, and its planted copies carry a Cyrillic
    letter there; candidates hold symbols no query has"""
    rng = np.random.default_rng(20261021)
    qa = GREEK + SHARED + CYRILLIC[:6] + HIGH[:2]
    qw = [6.0] * len(GREEK) + [3.0] * len(SHARED) + [0.5] * 6 + [1.0] * 2
    ca = CYRILLIC + SHARED + GREEK[:8] + HIGH[:2] + CAND_ONLY
    cw = [6.0] * len(CYRILLIC) + [2.0] * len(SHARED) + [0.5] * 8 + [1.0] * 2 + [1.5] * 2
    queries = []
    for j, ln in enumerate(QUERY_LENGTHS):
        q = list(draw(rng, qa, qw, ln))
        if ln >= 5:
            q[int(rng.integers(0, ln))] = QUERY_ONLY[j % 2]
        queries.append("".join(q))
    cands = [draw(rng, ca, cw, int(ln)) for ln in rng.integers(0, 71, size=307)]
    cands[0], cands[1] = draw(rng, ca, cw, 70), ""
    at = 3
    for q in queries:
        base = q.replace(QUERY_ONLY[0], CYRILLIC[9]).replace(QUERY_ONLY[1], CYRILLIC[11])
        for k in (0, 0, 1, 1, 2, 2, 3):
            cands[at % len(cands)] = str_edits(rng, base, k, CAND_ONLY[k % 2])
            at += 37
    have_q, have_c = {ch for q in queries for ch in q}, {ch for c in cands for ch in c}
    assert all(s in have_q and s not in have_c for s in QUERY_ONLY) and all(s in have_c and s not in have_q for s in CAND_ONLY)
    assert any(ord(ch) > 0xFFFF for ch in have_q & have_c)
    return queries, cands


def report(label, ok, detail):
    print(f"{label}: {detail}: {'ok' if ok else 'FAILED'}", flush=True)
    return 0 if ok else 1


def check_calls():
    off = os.environ.get("RF_JOIN") == "0"
    queries, cands = calls_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    assert qc.wide and cc.wide
    img = Image(queries, cands)
    bq = img(queries)
    data, offsets = rf.ragged(img(cands))
    fused_lens = [ln for ln in QUERY_LENGTHS if ln <= 64]
    assert len(fused_lens) == 7
    failures = 0
    # join
    for (metric, op), cutoffs in J.CUTOFFS.items():
        for cutoff in cutoffs:
            with PlanLines() as pl:
                got = J.got_triples(J.GPU[metric].BatchComparator.join(qc, cc, op, score_cutoff=cutoff))
            exp = J.Oracle(metric, op, cutoff, data, offsets).triples(bq)
            want = want_road("join", fused_lens, 1, off=off)
            failures += report(f"join {metric} op {op} cutoff {cutoff}", got == exp and len(exp) > 0 and pl.road == [want] * len(pl.road) and len(pl.road) >= 1,
                               f"{len(exp)} triples (got {len(got)}), plan {pl.road}, want {want}")
    # join_f64
    for metric, op, cutoff, weights in F.LENGTH_CASES:
        with PlanLines() as pl:
            got = F.got_triples(F.join(metric, qc, cc, op, cutoff, weights))
        exp = F.Oracle(metric, op, cutoff, data, offsets, weights).triples(bq)
        want = want_road("join_f64", fused_lens, 1, off=off)
        failures += report(f"join_f64 {metric} op {op} cutoff {cutoff} weights {weights}", got == exp and len(exp) > 0 and pl.road == [want] * len(pl.road) and len(pl.road) >= 1,
                           f"{len(exp)} triples (got {len(got)}), plan {pl.road}, want {want}")
    # join_topk
    for metric in ("levenshtein", "indel", "lcs_seq"):
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
            ora = T.TopkOracle(metric, op, None, data, offsets)
            with PlanLines() as pl:
                res = J.GPU[metric].BatchComparator.join_topk(qc, cc, 3, op)
            bad = T.mismatches(res, [ora.row(q, 3) for q in bq], 3)
            want = want_road("join_topk", fused_lens, 1, off=off)
            failures += report(f"join_topk {metric} op {op} k 3", not bad and pl.road == [want], f"rows differing {bad}, plan {pl.road}, want {want}")
    # join_topk_f64
    for metric, op in TF.FUSED_OPS:
        ora = TF.F64Oracle(metric, op, None, data, offsets)
        with PlanLines() as pl:
            res = TF.join(metric, qc, cc, 3, op)
        bad = TF.mismatches(res, [ora.row(q, 3) for q in bq], 3)
        want = want_road("join_topk_f64", fused_lens, 1, off=off)
        failures += report(f"join_topk_f64 {metric} op {op} k 3", not bad and pl.road == [want], f"rows differing {bad}, plan {pl.road}, want {want}")
    print("FAILURES", failures)
    return failures


def check_self():
    rng = np.random.default_rng(3)
    alphabet = GREEK[:4] + HIGH[:1]
    base = [draw(rng, alphabet, [1.0] * 5, 20) for _ in range(40)]
    rows = [base[int(i)] for i in rng.integers(0, 40, size=129)]  # duplicates
    for i in range(0, 129, 5):  # and near-duplicates
        rows[i] = str_edits(rng, rows[i], 1, GREEK[0])[:20].ljust(20, GREEK[1])
    corpus = rf.Corpus.from_list(rows)
    assert corpus.wide
    img = Image(rows)
    brows = img(rows)
    data, offsets = rf.ragged(brows)
    lev = rf.distance.levenshtein.BatchComparator
    ora = J.Oracle("levenshtein", N.OP_DISTANCE, 2, data, offsets)
    failures = 0
    for qi in (None, [40, 7, 3, 128, 7, 0, 5, 3, 77, 6, 4, 40, 99]):
        m = 129 if qi is None else len(qi)
        want = want_road("join", [20] * m, 0)
        with PlanLines() as pl:
            full = J.got_triples(lev.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, query_indices=qi))
            up = J.got_triples(lev.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, query_indices=qi, upper=True))
        exp, exp_up = ora.triples(brows, qi), ora.triples(brows, qi, upper=True)
        ok = full == exp and up == exp_up and 0 < len(exp_up) < len(exp) and pl.road == [want] * 4  # (count, then fetch: two calls each)
        failures += report(f"self-join rows {qi}", ok, f"{len(exp)} triples, {len(exp_up)} upper, plan {pl.road}, want {want}")
        tora = T.TopkOracle("levenshtein", N.OP_DISTANCE, None, data, offsets)
        rows_of = list(range(129)) if qi is None else qi
        for k in (1, 3):
            with PlanLines() as pl:
                res = lev.join_topk(corpus, corpus, k, N.OP_DISTANCE, query_indices=qi, no_self=True)
            exp_rows = [tora.row(brows[r], k, skip=r) for r in rows_of]
            bad = T.mismatches(res, exp_rows, k)
            own = sum(int(r in res[1][j, : int(res[2][j])].tolist()) for j, r in enumerate(rows_of))
            want = want_road("join_topk", [20] * m, 0)
            failures += report(f"self join_topk no_self k {k} rows {qi}", not bad and own == 0 and pl.road == [want], f"rows differing {bad}, {own} rows offered themselves, plan {pl.road}")
    print("FAILURES", failures)
    return failures


COMMON = [chr(0x4E00 + i) for i in range(254)]
RARE = [chr(0x5E00 + i) for i in range(40)] + [chr(0x1F680 + i) for i in range(6)]


def overflow_rows(seed, common=COMMON, rare=RARE, n_random=150):
    """rows over 254 common symbols, each at least three times, and 46 rare ones once each -- so the alphabet is the common symbols and the overflow class the
    rare ones, whatever the tie rule.  Pairs planted: rows 0 / 1 differ only in two DIFFERENT rare symbols at one position (distance 1, not 0); row 2 has no rare
    symbol and rows 3 / 4 are row 2 with a rare symbol substituted / inserted; the last row has 65 symbols."""
    rng = np.random.default_rng(seed)
    assert len(common) == 254 and len(rare) == 46
    rows = ["".join(common[(32 * r + i) % 254] for i in range(32)) for r in range(24)]  # every common symbol three times
    rows += [draw(rng, common, [1.0] * 254, int(ln)) for ln in rng.integers(1, 65, size=n_random)]
    stem = draw(rng, common, [1.0] * 254, 30)
    plain = draw(rng, common, [1.0] * 254, 40)
    head = [stem[:11] + rare[0] + stem[12:], stem[:11] + rare[1] + stem[12:], plain, plain[:7] + rare[2] + plain[8:], plain[:20] + rare[3] + plain[20:]]
    at = 4
    spots = list(range(30, 30 + 60))
    for r in spots:  # the other rare symbols: one each, one or two to a row, in random rows
        if at >= len(rare):
            break
        row = list(rows[r])
        for pos in rng.choice(len(row), size=min(1 + r % 2, len(row), len(rare) - at), replace=False):
            row[int(pos)] = rare[at]
            at += 1
        rows[r] = "".join(row)
    assert at == len(rare)
    rows = head + rows + [draw(rng, common, [1.0] * 254, 65)]
    counts = {}
    for row in rows:
        for ch in row:
            counts[ch] = counts.get(ch, 0) + 1
    assert all(counts.get(s, 0) >= 2 for s in common) and all(counts.get(s, 0) == 1 for s in rare) and len(counts) == 300
    return rows


def loop_join(cls, rows, positions, corpus, op, cutoff, f64):
    """the loop of single-query filter_many over rows[positions]: (position's row, candidate, score or its bits)"""
    out = []
    cache = {}
    for r in positions:
        if r not in cache:
            idx, sc = cls(rows[r]).filter_many(op, corpus, score_cutoff=cutoff)
            cache[r] = list(zip(idx.tolist(), F.bits(sc) if f64 else sc.tolist()))
        out += [(r, j, v) for j, v in cache[r]]
    return out


def loop_topk(cls, rows, positions, corpus, k, op):
    cache = {}
    for r in positions:
        if r not in cache:
            cache[r] = cls(rows[r]).topk(corpus, k, op)
    return [cache[r] for r in positions]


def four_calls(label, rows, qc, cc, positions, per_query_rows):
    """join, join_f64, join_topk, join_topk_f64 of rows[positions] (a corpus qc of `rows`) against cc equal the loop of single-query calls, and the plan lines
    show exactly the rows `per_query_rows` names (positions in `positions`), plus nothing else, per query"""
    lev = rf.distance.levenshtein.BatchComparator
    lens = [len(symbols(rows[r])) for j, r in enumerate(positions) if j not in per_query_rows]
    assert all(ln <= 64 for ln in lens) and lens and per_query_rows
    failures = 0
    qi = None if positions == list(range(len(rows))) else positions
    with PlanLines() as pl:
        got = J.got_triples(lev.join(qc, cc, N.OP_DISTANCE, score_cutoff=2, query_indices=qi))
    exp = loop_join(lev, rows, positions, cc, N.OP_DISTANCE, 2, False)
    want = want_road("join", lens, len(per_query_rows))
    failures += report(f"{label} join", got == exp and len(exp) > 0 and pl.road == [want] * 2, f"{len(exp)} triples (got {len(got)}), plan {pl.road}, want {want}")
    with PlanLines() as pl:
        got = F.got_triples(lev.join_f64(qc, cc, NS, score_cutoff=0.9, query_indices=qi))
    exp = loop_join(lev, rows, positions, cc, NS, 0.9, True)
    want = want_road("join_f64", lens, len(per_query_rows))
    failures += report(f"{label} join_f64", got == exp and len(exp) > 0 and pl.road == [want] * 2, f"{len(exp)} triples (got {len(got)}), plan {pl.road}, want {want}")
    with PlanLines() as pl:
        res = lev.join_topk(qc, cc, 3, N.OP_DISTANCE, query_indices=qi)
    bad = T.mismatches(res, loop_topk(lev, rows, positions, cc, 3, N.OP_DISTANCE), 3)
    want = want_road("join_topk", lens, len(per_query_rows))
    failures += report(f"{label} join_topk", not bad and pl.road == [want], f"rows differing {bad}, plan {pl.road}, want {want}")
    with PlanLines() as pl:
        res = lev.join_topk_f64(qc, cc, 2, NS, query_indices=qi)
    bad = TF.mismatches(res, loop_topk(lev, rows, positions, cc, 2, NS), 2)
    want = want_road("join_topk_f64", lens, len(per_query_rows))
    failures += report(f"{label} join_topk_f64", not bad and pl.road == [want], f"rows differing {bad}, plan {pl.road}, want {want}")
    return failures


def check_overflow():
    rows = overflow_rows(11)
    corpus = rf.Corpus.from_list(rows)
    assert corpus.wide
    rare = set(RARE)
    positions = list(range(len(rows)))
    per_query = {j for j, r in enumerate(positions) if len(rows[r]) > 64 or rare & set(rows[r])}
    assert 20 <= len(per_query) < 80 and len(rows) - 1 in per_query
    failures = four_calls("same handle", rows, corpus, corpus, positions, per_query)
    # the planted pairs, spelled out: two different rare symbols at one position are one substitution apart, not equal
    lev = rf.distance.levenshtein.BatchComparator
    got = set(J.got_triples(lev.join(corpus, corpus, N.OP_DISTANCE, score_cutoff=2, query_indices=[0, 1, 2, 3, 4])))
    pairs = {(0, 0, 0), (0, 1, 1), (1, 0, 1), (1, 1, 0), (2, 2, 0), (2, 3, 1), (2, 4, 1), (3, 2, 1), (3, 3, 0), (3, 4, 2), (4, 2, 1), (4, 3, 2), (4, 4, 0)}
    failures += report("planted pairs", pairs <= got, f"missing {sorted(pairs - got)}")
    print("FAILURES", failures)
    return failures


def check_across():
    failures = 0
    rare = set(RARE)
    over = overflow_rows(11)
    # 1. the queries' corpus has the overflow class, the scanned one does not: copies of the rows over 200 of the common symbols, rare symbols replaced
    rng = np.random.default_rng(12)
    small = [row.translate({ord(s): COMMON[i % 200] for i, s in enumerate(RARE + COMMON[200:])}) for row in over[:120]]
    small = [str_edits(rng, row, j % 3, COMMON[5]) for j, row in enumerate(small)]
    sc = rf.Corpus.from_list(small)
    qc = rf.Corpus.from_list(over)
    assert sc.wide and qc.wide and len({ch for row in small for ch in row}) <= 254
    positions = list(range(0, len(over), 2)) + [len(over) - 1]
    per_query = {j for j, r in enumerate(positions) if len(over[r]) > 64 or rare & set(over[r])}
    failures += four_calls("overflow on the queries' side", over, qc, sc, positions, per_query)
    # 2. the reverse: the queries' corpus has 100-odd symbols, three of them rare over there -- each several times here, so this corpus has no overflow class
    pool = COMMON[:100] + RARE[:3]
    queries = [draw(rng, pool, [1.0] * 100 + [0.4] * 3, int(ln)) for ln in rng.integers(1, 65, size=60)]
    queries[0], queries[1] = over[0], over[2]  # (a copy of a row with a rare symbol; a copy of one without)
    queries.append(draw(rng, COMMON[:100], [1.0] * 100, 65))
    qs = rf.Corpus.from_list(queries)
    assert qs.wide and len({ch for row in queries for ch in row}) <= 254 and all(sum(row.count(s) for row in queries) >= 2 for s in RARE[:3])
    positions = list(range(len(queries)))
    per_query = {j for j in positions if len(queries[j]) > 64 or rare & set(queries[j])}
    assert 5 <= len(per_query) < 40
    failures += four_calls("overflow on the scanned side", queries, qs, qc, positions, per_query)
    # 3. both: a second corpus over the same common symbols whose rare symbols are partly the first one's, partly its own
    rare2 = RARE[:20] + [chr(0x6E00 + i) for i in range(26)]
    over2 = overflow_rows(13, rare=rare2)
    qc2 = rf.Corpus.from_list(over2)
    positions = list(range(0, len(over2), 2)) + [len(over2) - 1]
    per_query = {j for j, r in enumerate(positions) if len(over2[r]) > 64 or (rare | set(rare2)) & set(over2[r])}
    failures += four_calls("overflow on both sides", over2, qc2, qc, positions, per_query)
    print("FAILURES", failures)
    return failures


def check_mixed():
    failures = 0
    rng = np.random.default_rng(14)
    latin = [chr(c) for c in range(0x61, 0x7B)] + ["é", "ü", "ñ", "ÿ"]
    lw = [1.0] * len(latin)
    # 1. byte queries against a `char` corpus: a byte is the code point
    qs = [draw(rng, latin, lw, ln) for ln in QUERY_LENGTHS]
    cands = [draw(rng, latin + GREEK[:6], lw + [0.7] * 6, int(ln)) for ln in rng.integers(0, 71, size=200)]
    for j, q in enumerate(qs):
        cands[3 + 11 * j], cands[4 + 11 * j] = q, str_edits(rng, q, 2, GREEK[0])
    bq = [q.encode("latin-1") for q in qs]
    qc, cc = rf.Corpus.from_list(bq), rf.Corpus.from_list(cands)
    assert not qc.wide and cc.wide
    img = Image(bq, cands)
    data, offsets = rf.ragged(img(cands))
    fused_lens = [ln for ln in QUERY_LENGTHS if ln <= 64]
    lev = rf.distance.levenshtein.BatchComparator

    def both(label, qc, cc, iq, data, offsets):
        bad = 0
        with PlanLines() as pl:
            got = J.got_triples(lev.join(qc, cc, N.OP_DISTANCE, score_cutoff=3))
        exp = J.Oracle("levenshtein", N.OP_DISTANCE, 3, data, offsets).triples(iq)
        want = want_road("join", fused_lens, 1)
        bad += report(f"{label} join", got == exp and len(exp) >= 16 and pl.road == [want] * 2, f"{len(exp)} triples (got {len(got)}), plan {pl.road}, want {want}")
        ora = TF.F64Oracle("indel", NS, None, data, offsets)
        with PlanLines() as pl:
            res = TF.join("indel", qc, cc, 3, NS)
        rows = TF.mismatches(res, [ora.row(q, 3) for q in iq], 3)
        want = want_road("join_topk_f64", fused_lens, 1)
        bad += report(f"{label} join_topk_f64", not rows and pl.road == [want], f"rows differing {rows}, plan {pl.road}, want {want}")
        return bad

    failures += both("bytes x char", qc, cc, img(bq), data, offsets)
    # 2. `char` queries of symbols <= 0xFF against a byte corpus
    wq = rf.Corpus.from_u32_list(qs)
    bcands = [draw(rng, latin, lw, int(ln)) for ln in rng.integers(0, 71, size=200)]
    for j, q in enumerate(qs):
        bcands[3 + 11 * j], bcands[4 + 11 * j] = q, str_edits(rng, q, 2, "z")
    bc = rf.Corpus.from_list(bcands)
    assert wq.wide and not bc.wide
    img = Image(qs, bcands)
    data, offsets = rf.ragged(img(bcands))
    failures += both("char x bytes", wq, bc, img(qs), data, offsets)
    # 3. one `char` row with a symbol above 0xFF against a byte corpus: the per-query road's error, outputs untouched; the rows before it are not answered either
    wq2 = rf.Corpus.from_list(qs[:5] + [qs[3][:10] + GREEK[0] + qs[3][11:]] + qs[5:7])
    assert wq2.wide
    args = rf.Args().score_cutoff(3).to_c(False)
    oq, oi, sc, cnt = np.full(64, 77, dtype=np.uint64), np.full(64, 77, dtype=np.uint64), np.full(64, 77, dtype=np.uint32), np.full(1, 77, dtype=np.uint64)
    with PlanLines() as pl:
        st = N.lib().rf_join_u32(N.LEVENSHTEIN, wq2._h, None, 8, bc._h, N.OP_DISTANCE, C.byref(args), 0, 0, 0, 64, oq.ctypes.data, oi.ctypes.data, sc.ctypes.data,
                                 cnt.ctypes.data_as(C.POINTER(C.c_uint64)), N.JOIN_BY_QUERY, None)
    want = want_road("join", [0, 1, 5, 32, 33, 64, 64], 1)
    ok = st == N.RF_ERR_UNSUPPORTED and (oq == 77).all() and (oi == 77).all() and (sc == 77).all() and (cnt == 77).all() and pl.road == [want]
    failures += report("a symbol above 0xFF against bytes, join", ok, f"status {st}, plan {pl.road}, want {want}")
    args = rf.Args().to_c(False)
    ts, ti, tc = np.full((8, 2), 77, dtype=np.uint32), np.full((8, 2), 77, dtype=np.uint64), np.full(8, 77, dtype=np.uint32)
    with PlanLines() as pl:
        st = N.lib().rf_join_topk_u32(N.LEVENSHTEIN, wq2._h, None, 8, bc._h, N.OP_DISTANCE, C.byref(args), 0, 2, 0, ts.ctypes.data, ti.ctypes.data, tc.ctypes.data, None)
    want = want_road("join_topk", [0, 1, 5, 32, 33, 64, 64], 1)
    ok = st == N.RF_ERR_UNSUPPORTED and (ts == 77).all() and (ti == 77).all() and (tc == 77).all() and pl.road == [want]
    failures += report("a symbol above 0xFF against bytes, join_topk", ok, f"status {st}, plan {pl.road}, want {want}")
    print("FAILURES", failures)
    return failures


def check_batch():
    assert os.environ.get("RF_JOIN_BATCH") == "8", "run with RF_JOIN_BATCH=8"
    queries, cands = calls_case()
    qc, cc = rf.Corpus.from_list(queries), rf.Corpus.from_list(cands)
    img = Image(queries, cands)
    bq = img(queries)
    data, offsets = rf.ragged(img(cands))
    rng = np.random.default_rng(5)
    lev = rf.distance.levenshtein.BatchComparator
    ora = J.Oracle("levenshtein", N.OP_DISTANCE, 3, data, offsets)
    tora = T.TopkOracle("levenshtein", N.OP_DISTANCE, None, data, offsets)
    failures = 0
    for m in range(1, 18):
        qi = rng.integers(0, 7, size=m)  # (rows 0..6: the fusable ones; repeats, any order)
        lens = [QUERY_LENGTHS[int(i)] for i in qi]
        with PlanLines() as pl:
            got = J.got_triples(lev.join(qc, cc, N.OP_DISTANCE, score_cutoff=3, query_indices=qi))
            res = lev.join_topk(qc, cc, 2, N.OP_DISTANCE, query_indices=qi)
        exp = ora.triples(bq, qi)
        # (the positions in Q come back as row indices: query_base + qidx)
        bad = T.mismatches(res, [tora.row(bq[int(i)], 2) for i in qi], 2)
        want = [want_road("join", lens, 0, batch=8)] * 2 + [want_road("join_topk", lens, 0, batch=8)]
        failures += report(f"m={m} rows {qi.tolist()}", got == exp and not bad and pl.road == want, f"{len(exp)} triples, top-k rows differing {bad}, plan {pl.road}, want {want}")
    print("FAILURES", failures)
    return failures


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    fn = {"calls": check_calls, "self": check_self, "overflow": check_overflow, "across": check_across, "mixed": check_mixed, "batch": check_batch}[sys.argv[1]]
    sys.exit(1 if fn() else 0)
