"""damerau_levenshtein::BatchComparator on the device (rf_damerau.hip), bit-exact against tests/dl_reference.py: the reference's known answers,
parity over corpus shapes x query lengths x ops x cutoffs (the register kernels, the LDS rows with 8- and 16-bit fields, the global rows), every
result road, two pack-time layouts through child processes, a randomized differential test, the steps of the plan from the query's side (149 / 150, 254 / 255, and with
a 255-symbol candidate 74 / 75, 99 / 100, 149 / 150, 299 / 300) and the field limit (65 534 symbols answered on either side, 65 535 refused with the output untouched).
Here every wavefront walks ONE tile; several tiles per wavefront of each of these kernels: tests/multitile_rowdp_check.py, mode "damerau" (started by tests/test_gpu_parity.py).

The inputs are chosen so that a kernel computing a NEIGHBOURING metric fails: near-duplicates are planted by "swap two adjacent symbols and insert
a random symbol between them" (four times, clipped to 64) -- one transposition-with-insertion costs 2 here and 3 in OSA -- and the tests assert from the
restatement alone that at least half of the planted rows and at least 5 % of the random 4-symbol rows have DL < OSA (measured on the CPU when the
test was written: 0.98 of planted rows over 62 symbols, 0.61 over 4 symbols, 0.115 of random 4-symbol rows of 40..64 symbols)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

import dl_reference as R
import textbook

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DL = rf.distance.damerau_levenshtein
OPS = (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY)
KNOWN = [("", "", 0), ("aaaa", "", 4), ("aaaa", "aaaa", 0), ("aaaa", "aaa", 1), ("aaaa", "aaab", 1), ("abaa", "baaa", 1), ("aaaa", "bbbb", 4), ("CA", "ABC", 2)]
KNOWN_NORM_SIM = [1.0, 0.75, 0.75, 0.75, 0.0]
KNOWN_CHARS = [("Иванко", "Петрунко", 5), ("ИвaнкoIvan", "Петрунко", 10)]


def _planted(rng, q, sym, clip=64):
    c = list(q)
    for _ in range(4):
        if len(c) < 2:
            break
        p = int(rng.integers(len(c) - 1))
        c[p], c[p + 1] = c[p + 1], c[p]
        c.insert(p + 1, int(rng.integers(sym)))
    return c[:clip]


def _rand(rng, length, sym):
    return [int(v) for v in rng.integers(sym, size=length)]


def _frac_below_osa(q, rows):
    return float(np.mean([R.dl_pair(q, c) < textbook.osa(q, c) for c in rows]))


def _bytes_corpus(cands, base=48):
    """candidates as lists of symbol ids -> (Corpus of bytes, rows, lens); ids are shifted to printable bytes so that renaming has something to do"""
    corpus = rf.Corpus.from_list([bytes(base + v for v in c) for c in cands])
    rows, lens = R.pad_rows([[base + v for v in c] for c in cands])
    return corpus, rows, lens


def _cutoffs(op, len1, lens):
    mx = max(len1, int(lens.max()) if len(lens) else 0)
    gap = abs(len1 - int(np.median(lens))) if len(lens) else 0
    if op == N.OP_DISTANCE:
        return sorted({0, 3, mx // 3, mx // 2 + 1, max(gap - 1, 0), gap + 2, mx + 5})
    if op == N.OP_SIMILARITY:
        return sorted({0, 1, mx // 2, max(mx - 3, 0), mx, mx + 5})  # the upper ones leave maximum - cutoff < |len1 - len2|: the similarity-None case
    return [0.0, 0.3, 0.5, 0.9, 1.0]


def _eq(got, exp, what):
    if exp.dtype == np.uint32:
        bad = np.nonzero(got != exp)[0]
    else:
        bad = np.nonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[0]
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:5]}: got {got[bad[:5]]}, expected {exp[bad[:5]]}"


def _parity(q_bytes, corpus, rows, lens, what, ops=OPS, cutoffs=True):
    bc = DL.BatchComparator(q_bytes)
    qv = list(q_bytes)
    dist = R.dl_many(qv, rows, lens)
    for op in ops:
        _eq(bc.many(op, corpus), R.ops(op, qv, rows, lens, None, dist), f"{what} op {op}")
        for c in _cutoffs(op, len(qv), lens) if cutoffs else ():
            _eq(bc.many(op, corpus, score_cutoff=c), R.ops(op, qv, rows, lens, c, dist), f"{what} op {op} cutoff {c}")
    return dist


def test_normalized_cutoffs_that_equal_a_produced_quotient():
    """f64 cutoffs that ARE a candidate's d / maximum (or 1 - d / maximum) and the doubles on either side of it: 200 candidates of 0..40 symbols, a query of 24,
    at most 12 of the produced values by rank (the smallest and the largest among them), against tests/dl_reference.py called WITH the cutoff -- every value
    bit-equal, every None a None -- through many, filter_many and top-k.  The round decimals of _cutoffs() almost never equal a score, so they cannot tell
    `<=` from `<` in emit_fin's compare."""
    rng = np.random.default_rng(2406)
    q = _rand(rng, 24, 12)
    cands = [_planted(rng, q, 12) if i % 4 == 0 else _rand(rng, int(rng.integers(0, 41)), 12) for i in range(200)]
    cands[4] = list(q)
    corpus, rows, lens = _bytes_corpus(cands)
    qb = bytes(48 + v for v in q)
    qv = list(qb)
    bc = DL.BatchComparator(qb)
    dist = R.dl_many(qv, rows, lens)
    told_apart = 0
    for op in (N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY):
        full = R.ops(op, qv, rows, lens, None, dist)
        vals = np.unique(full)
        picked = vals[np.unique(np.linspace(0, len(vals) - 1, num=12).round().astype(int))]
        assert len(picked) >= 8 and picked[0] == vals[0] and picked[-1] == vals[-1] and 0.0 in vals.tolist() + (1.0 - vals).tolist()
        for v in picked:
            triple = [float(np.nextafter(v, -1.0)), float(v), float(np.nextafter(v, 2.0))]
            kept = []
            for c in triple:
                exp = R.ops(op, qv, rows, lens, c, dist)
                kept.append(int(np.count_nonzero(~np.isnan(exp))))
                got = bc.many(op, corpus, score_cutoff=c)
                same = (np.isnan(got) & np.isnan(exp)) | (got.view(np.uint64) == exp.view(np.uint64))
                assert same.all(), (op, c, np.nonzero(~same)[0][:5], got[~same][:5], exp[~same][:5])
                some = np.nonzero(~np.isnan(exp))[0]
                idx, sc = bc.filter_many(op, corpus, score_cutoff=c)
                assert idx.tolist() == some.tolist() and sc.view(np.uint64).tolist() == exp[some].view(np.uint64).tolist(), (op, c)
                best = some[np.lexsort((some, exp[some] if op == N.OP_NORMALIZED_DISTANCE else -exp[some]))][:16]
                scores, at = bc.topk(corpus, 16, op=op, score_cutoff=c)
                assert at.tolist() == best.tolist() and scores.view(np.uint64).tolist() == exp[best].view(np.uint64).tolist(), (op, c)
            told_apart += kept[0] != kept[2]
    assert told_apart >= 16  # (the neighbours of a produced value keep different numbers of candidates: a flipped compare shows)


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers_through_one_and_through_a_corpus():
    for a, b, d in KNOWN:
        assert DL.distance(a.encode(), b.encode()) == d and DL.BatchComparator(a.encode()).distance(b.encode()) == d, (a, b)
    for (a, b, d), ns in zip(KNOWN[2:7], KNOWN_NORM_SIM):
        assert DL.normalized_similarity(a.encode(), b.encode(), score_cutoff=0.0) == ns, (a, b)
    for a, b, d in KNOWN_CHARS:
        assert DL.distance(a, b) == d and DL.distance(b, a) == d, (a, b)
    # ... and as corpora: every known second string under every known first string, bytes and chars
    seconds = sorted({b for _, b, _ in KNOWN} | {a for a, _, _ in KNOWN})
    corpus = rf.Corpus.from_list([s.encode() for s in seconds])
    for a in sorted({a for a, _, _ in KNOWN}):
        got = DL.BatchComparator(a.encode()).distance_many(corpus)
        assert got.tolist() == [R.dl_pair(a, s) for s in seconds], a
    for a, b, d in KNOWN:
        assert int(DL.BatchComparator(a.encode()).distance_many(corpus)[seconds.index(b)]) == d
    chars = ["Иванко", "Петрунко", "ИвaнкoIvan", "", "Ивнако", "CA", "ABC"]
    wide = rf.Corpus.from_u32_list(chars)
    for a in chars:
        assert DL.BatchComparator(a).distance_many(wide).tolist() == [R.dl_pair(a, s) for s in chars], a
    # the neighbour that is not a metric answers differently on the textbook pair
    assert DL.distance(b"CA", b"ABC") == 2
    assert rf.distance.osa.distance(b"CA", b"ABC") == 3


# ------------------------------------------------------------------------------------------------ parity over shapes x query lengths
QLENS = [0, 1, 15, 16, 17, 32, 33, 63, 64, 65, 200, 300, 700]


def _shape_rows(shape, rng, q, sym):
    """random rows + planted near-duplicates of the query, in the length law of the shape"""
    n_rand, n_plant = (700, 260) if len(q) <= 65 else (200, 70)
    if shape == "single64":
        rows = [_rand(rng, 64, sym) for _ in range(n_rand)]
        plant = [(_planted(rng, q, sym) + _rand(rng, 64, sym))[:64] for _ in range(n_plant)]
    elif shape == "ragged":
        rows = [_rand(rng, int(rng.integers(1, 65)), sym) for _ in range(n_rand)]
        plant = [_planted(rng, q, sym) or _rand(rng, 1, sym) for _ in range(n_plant)]
    else:  # bucketed: whole tiles of a few lengths + leftovers of every length (mixed tiles) + zero-length rows
        rows = [_rand(rng, L, sym) for L in (0, 5, 17, 40, 64) for _ in range(64 + 9)] + [_rand(rng, int(rng.integers(0, 65)), sym) for _ in range(n_rand // 2)]
        plant = [_planted(rng, q, sym) for _ in range(n_plant)]
    return rows, plant


@pytest.mark.parametrize("qlen", QLENS)
@pytest.mark.parametrize("shape", ["ragged", "single64", "bucketed"])
def test_parity_over_shapes_and_query_lengths(shape, qlen):
    rng = np.random.default_rng(100 * qlen + len(shape))
    sym = 62
    q = _rand(rng, qlen, sym)
    rows, plant = _shape_rows(shape, rng, q, sym)
    if 16 <= qlen <= 64:  # conditions on the INPUTS, from the restatement alone: these rows tell this metric from OSA
        assert _frac_below_osa(q, plant[:80]) >= 0.5
    order = rng.permutation(len(rows) + len(plant))
    cands = [(rows + plant)[i] for i in order]
    corpus, r, lens = _bytes_corpus(cands)
    few_ops = qlen > 65  # the long queries: every op, fewer cutoffs (the reference takes its time)
    dist = _parity(bytes(48 + v for v in q), corpus, r, lens, f"{shape} query {qlen}", cutoffs=not few_ops)
    if few_ops:
        bc = DL.BatchComparator(bytes(48 + v for v in q))
        qv = [48 + v for v in q]
        _eq(bc.many(N.OP_DISTANCE, corpus, score_cutoff=qlen - 40), R.ops(N.OP_DISTANCE, qv, r, lens, qlen - 40, dist), "long distance cutoff")
        _eq(bc.many(N.OP_SIMILARITY, corpus, score_cutoff=30), R.ops(N.OP_SIMILARITY, qv, r, lens, 30, dist), "long similarity cutoff")
        _eq(bc.many(N.OP_NORMALIZED_SIMILARITY, corpus, score_cutoff=0.1), R.ops(N.OP_NORMALIZED_SIMILARITY, qv, r, lens, 0.1, dist), "long normalized cutoff")


def test_random_four_symbol_rows_differ_from_osa():
    rng = np.random.default_rng(5)
    q = _rand(rng, 64, 4)
    cands = [_rand(rng, int(rng.integers(40, 65)), 4) for _ in range(640)]
    assert _frac_below_osa(q, cands[:300]) >= 0.05  # a condition on the inputs
    corpus, rows, lens = _bytes_corpus(cands)
    dist = _parity(bytes(48 + v for v in q), corpus, rows, lens, "random 4-symbol rows", ops=(N.OP_DISTANCE,))
    osa = rf.distance.osa.BatchComparator(bytes(48 + v for v in q)).distance_many(corpus)
    assert (dist <= osa).all() and (dist < osa).mean() >= 0.05


def test_one_long_candidate_forces_the_wide_cell():
    rng = np.random.default_rng(6)
    q = _rand(rng, 20, 4)
    cands = [_rand(rng, int(rng.integers(0, 40)), 4) for _ in range(200)] + [_planted(rng, q, 4) for _ in range(60)]
    cands.insert(77, (_planted(rng, q, 4) + _rand(rng, 400, 4))[:400])
    corpus, rows, lens = _bytes_corpus(cands)
    _parity(bytes(48 + v for v in q), corpus, rows, lens, "400-symbol candidate")
    # the field-width edge from the device's side: the longest string at 254 (8-bit fields) and 255 (16-bit fields)
    for edge in (254, 255):
        cands[77] = _rand(rng, edge, 4)
        corpus, rows, lens = _bytes_corpus(cands)
        _parity(bytes(48 + v for v in q), corpus, rows, lens, f"{edge}-symbol candidate", ops=(N.OP_DISTANCE, N.OP_NORMALIZED_SIMILARITY), cutoffs=False)


def test_chars_corpus_parity():
    rng = np.random.default_rng(8)
    alphabet = [ord(c) for c in "абвгдежзийклмнопрстуфхцчшщъыьэюяAbc1"]
    q = [alphabet[i] for i in rng.integers(len(alphabet), size=23)]
    cands = [[alphabet[i] for i in rng.integers(len(alphabet), size=int(rng.integers(0, 50)))] for _ in range(300)]
    cands += [[alphabet[v] for v in _planted(rng, [alphabet.index(s) for s in q], len(alphabet))] for _ in range(100)]
    corpus = rf.Corpus.from_u32_list(["".join(map(chr, c)) for c in cands])
    rows, lens = R.pad_rows(cands)
    bc = DL.BatchComparator("".join(map(chr, q)))
    dist = R.dl_many(q, rows, lens)
    for op in OPS:
        _eq(bc.many(op, corpus), R.ops(op, q, rows, lens, None, dist), f"chars op {op}")
    _eq(bc.many(N.OP_DISTANCE, corpus, score_cutoff=6), R.ops(N.OP_DISTANCE, q, rows, lens, 6, dist), "chars cutoff")
    # a query symbol the corpus does not hold never matches
    q2 = q[:10] + [0x4E2D] + q[10:]
    _eq(DL.BatchComparator("".join(map(chr, q2))).distance_many(corpus), R.ops(N.OP_DISTANCE, q2, rows, lens), "chars, absent symbol")


# ------------------------------------------------------------------------------------------------ the query-side edges of the plan
# (query length, a 255-symbol candidate inserted, the plan): plan() (rf_api_scan.hip) picks the cell width from the longest string of the call -- 8-bit fields up
# to 254 symbols, 16-bit from 255 on -- and the wavefronts per workgroup from the row of len1 x 64 cells (4 bytes narrow, 8 wide) within 150 KiB of LDS less
# len1 + 16: waves = min(4, (153600 - len1 - 16) // row_bytes), the global strip when not even one row fits.
#   narrow  149: 153435 // 38144 = 4    150: 153434 // 38400 = 3    254: 153330 // 65024 = 2
#   wide     74: 153510 // 37888 = 4     75: 153509 // 38400 = 3     99: 153485 // 50688 = 3    100: 153484 // 51200 = 2    149: 153435 // 76288 = 2
#           150: 153434 // 76800 = 1    255: 153329 // 130560 = 1   299: 153088 + 299 + 16 = 153403 <= 153600, one row    300: 153600 + 316 > 153600: global
DL_EDGE_LEGS = [(149, False, "lds8 x4"), (150, False, "lds8 x3"), (254, False, "lds8 x2"), (255, False, "lds16 x1"),
                (74, True, "lds16 x4"), (75, True, "lds16 x3"), (99, True, "lds16 x3"), (100, True, "lds16 x2"), (149, True, "lds16 x2"), (150, True, "lds16 x1"),
                (299, True, "lds16 x1"), (300, True, "global16")]


def _dl_plan(len1, longest):
    """the plan of a damerau_levenshtein launch, with the arithmetic of tests/multitile_rowdp_check.py dl_waves"""
    import multitile_rowdp_check as M

    wide = max(len1, longest) > 254
    if not wide and len1 <= 64:
        return "reg"
    cells = 16 if wide else 8
    if max(len1, 1) * 64 * (8 if wide else 4) + len1 + 16 > M.LDS_BUDGET:
        return f"global{cells}"
    return f"lds{cells} x{M.dl_waves(len1, longest)}"


@pytest.mark.parametrize("qlen,wide_candidate,plan", DL_EDGE_LEGS)
def test_query_side_edges_of_the_plan(qlen, wide_candidate, plan):
    """about 200 candidates of up to 64 symbols and 60 planted near-duplicates, one ragged corpus law for every leg; with `wide_candidate` one 255-symbol
    candidate among them makes the cells wide"""
    rng = np.random.default_rng(4242)
    sym = 62
    cands = [_rand(rng, int(rng.integers(0, 65)), sym) for _ in range(200)]
    q = _rand(np.random.default_rng(qlen), qlen, sym)
    plant = [_planted(rng, q[:60], sym) for _ in range(60)]  # (planted in the query's first 60 symbols: the clip to 64 leaves every swap in)
    assert _frac_below_osa(q, plant[:12]) >= 0.5  # the inputs: the planted rows tell this metric from OSA
    cands = [(cands + plant)[i] for i in rng.permutation(len(cands) + len(plant))]
    dist = R.dl_many(q, *R.pad_rows(cands))
    if wide_candidate:
        long_one = (_planted(rng, q, sym, clip=255) + _rand(rng, 255, sym))[:255]
        cands.insert(77, long_one)
        dist = np.insert(dist, 77, R.dl_pair(q, long_one))  # (the vectorised form walks every column of the longest row: the per-pair form for this one)
    longest = max(len(c) for c in cands)
    assert longest == (255 if wide_candidate else 64) and _dl_plan(qlen, longest) == plan  # the inputs: this leg is the plan it says
    corpus, rows, lens = _bytes_corpus(cands)
    bc = DL.BatchComparator(bytes(48 + v for v in q))
    qv = [48 + v for v in q]
    for op in OPS:
        _eq(bc.many(op, corpus), R.ops(op, qv, rows, lens, None, dist), f"query {qlen} ({plan}) op {op}")
        for c in _cutoffs(op, qlen, lens):
            _eq(bc.many(op, corpus, score_cutoff=c), R.ops(op, qv, rows, lens, c, dist), f"query {qlen} ({plan}) op {op} cutoff {c}")


def test_the_plans_of_the_query_side_edges_change_where_they_say():
    """host arithmetic only: each pair of neighbouring lengths sits on either side of a step of the plan"""
    plans = {(q, w): p for q, w, p in DL_EDGE_LEGS}
    for lo, hi, w in ((149, 150, False), (254, 255, False), (74, 75, True), (99, 100, True), (149, 150, True), (299, 300, True)):
        assert plans[(lo, w)] != plans[(hi, w)], (lo, hi, w)
        assert _dl_plan(lo, 255 if w else 64) == plans[(lo, w)] and _dl_plan(hi, 255 if w else 64) == plans[(hi, w)]
    assert {p for (_, w), p in plans.items() if w} == {"lds16 x4", "lds16 x3", "lds16 x2", "lds16 x1", "global16"}


# ------------------------------------------------------------------------------------------------ the field limit: 65 534 symbols accepted, 65 535 refused
FIELD_MAX = 65_534  # the largest length the 16-bit fields of a cell hold (rf_dl_cell.hpp); 65 535 is their "infinity"


def _limit_parity(q, cands, what):
    dist = np.array([R.dl_pair(q, c) for c in cands], dtype=np.int64)  # (per pair: a few hundred thousand cells each)
    corpus, rows, lens = _bytes_corpus(cands, base=0)
    bc = DL.BatchComparator(bytes(q))
    for op in OPS:
        _eq(bc.many(op, corpus), R.ops(op, q, rows, lens, None, dist), f"{what} op {op}")
    for op, c in ((N.OP_DISTANCE, FIELD_MAX), (N.OP_DISTANCE, FIELD_MAX - 1), (N.OP_DISTANCE, int(dist.min())), (N.OP_SIMILARITY, 1), (N.OP_SIMILARITY, 0),
                  (N.OP_NORMALIZED_DISTANCE, 1.0), (N.OP_NORMALIZED_SIMILARITY, 1e-4)):
        _eq(bc.many(op, corpus, score_cutoff=c), R.ops(op, q, rows, lens, c, dist), f"{what} op {op} cutoff {c}")
    return dist


def test_a_query_of_65534_symbols():
    rng = np.random.default_rng(65534)
    q = [int(v) for v in rng.integers(1, 5, size=FIELD_MAX)]
    cands = [[], q[100:108], [q[201], q[200], 9, q[203]]]  # nothing, a piece of the query, a piece with a swap and a symbol the query does not hold
    assert len(q) == FIELD_MAX and max(len(c) for c in cands) <= 8
    dist = _limit_parity(q, cands, "query of 65534")
    assert int(dist.max()) == FIELD_MAX and len(set(dist.tolist())) >= 3  # the largest value a field can hold is a result


def test_candidates_of_65534_and_65533_symbols():
    rng = np.random.default_rng(65533)
    q = [1, 2, 3]
    cands = [[9] * FIELD_MAX, [int(v) for v in rng.integers(1, 5, size=FIELD_MAX - 1)], [int(v) for v in rng.integers(1, 5, size=40)]]
    assert [len(c) for c in cands] == [FIELD_MAX, FIELD_MAX - 1, 40]
    dist = _limit_parity(q, cands, "candidates of 65534")
    assert int(dist[0]) == FIELD_MAX and len(set(dist.tolist())) >= 3


@pytest.mark.parametrize("side", ["query", "candidate"])
def test_a_string_of_65535_symbols_is_refused_with_the_output_untouched(side):
    import ctypes as C

    rng = np.random.default_rng(65535)
    long_one = bytes(int(v) for v in rng.integers(1, 5, size=FIELD_MAX + 1))
    short = [bytes(int(v) for v in rng.integers(1, 5, size=int(rng.integers(0, 9)))) for _ in range(70)]
    q, cands = (long_one, short) if side == "query" else (bytes([1, 2, 3]), short[:30] + [long_one] + short[30:])
    assert max(len(q), max(len(c) for c in cands)) == FIELD_MAX + 1
    corpus = rf.Corpus.from_list(cands)
    bc = DL.BatchComparator(q)
    a = N.RfArgs()
    N.lib().rf_args_default(C.byref(a))
    out = np.full(len(cands), 0xA5A5A5A5, dtype=np.uint32)
    assert N.lib().rf_many_u32(bc._h, corpus._h, N.OP_DISTANCE, C.byref(a), out.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_UNSUPPORTED
    assert "65535" in N.lib().rf_last_error().decode() and (out == 0xA5A5A5A5).all()
    outf = np.full(len(cands), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert N.lib().rf_many_f64(bc._h, corpus._h, N.OP_NORMALIZED_SIMILARITY, C.byref(a), outf.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_UNSUPPORTED
    assert (outf == 0xA5A5A5A5A5A5A5A5).all()
    for call in (lambda: bc.distance_many(corpus), lambda: bc.topk(corpus, 5), lambda: bc.filter_many(N.OP_DISTANCE, corpus, score_cutoff=3)):
        with pytest.raises(N.RfError) as e:
            call()
        assert e.value.status == N.RF_ERR_UNSUPPORTED
    # one symbol fewer on that side is answered
    if side == "query":
        q = q[:-1]
    else:
        cands[30] = cands[30][:-1]
        corpus = rf.Corpus.from_list(cands)
    got = DL.BatchComparator(q).distance_many(corpus)
    i = 5 if side == "query" else 30
    assert int(got[i]) == R.dl_pair(list(q), list(cands[i]))


# ------------------------------------------------------------------------------------------------ every road
def _road_case(seed=11, n=3000):
    rng = np.random.default_rng(seed)
    q = _rand(rng, 40, 62)
    plant = [_planted(rng, q, 62) for _ in range(n // 10)]
    assert _frac_below_osa(q, plant[:60]) >= 0.5  # the road inputs, too, tell this metric from OSA
    cands = [_rand(rng, int(rng.integers(0, 65)), 62) for _ in range(n)] + plant
    cands = [cands[i] for i in rng.permutation(len(cands))]
    return q, cands


@pytest.mark.parametrize("k", [4, 100])
def test_topk_equals_a_sort_of_the_dense_result(k):
    q, cands = _road_case()
    corpus, rows, lens = _bytes_corpus(cands)
    bc = DL.BatchComparator(bytes(48 + v for v in q))
    qv = [48 + v for v in q]
    for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_DISTANCE, 9), (N.OP_SIMILARITY, None), (N.OP_NORMALIZED_SIMILARITY, 0.5)):
        exp = R.ops(op, qv, rows, lens, cutoff)
        some = np.nonzero(exp != R.NONE_U32)[0] if exp.dtype == np.uint32 else np.nonzero(~np.isnan(exp))[0]
        desc = op in (N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY)
        order = sorted(some.tolist(), key=lambda i: ((-float(exp[i]) if desc else float(exp[i])), i))[:k]
        scores, idx = bc.topk(corpus, k, op=op, score_cutoff=cutoff)
        assert idx.tolist() == order and scores.tolist() == exp[order].tolist(), (op, cutoff)


def test_filter_many_equals_nonzero_of_the_somes():
    q, cands = _road_case(12)
    corpus, rows, lens = _bytes_corpus(cands)
    bc = DL.BatchComparator(bytes(48 + v for v in q))
    qv = [48 + v for v in q]
    for op, cutoff in ((N.OP_DISTANCE, 9), (N.OP_DISTANCE, 30), (N.OP_SIMILARITY, 30), (N.OP_NORMALIZED_DISTANCE, 0.3)):
        exp = R.ops(op, qv, rows, lens, cutoff)
        some = np.nonzero(exp != R.NONE_U32)[0] if exp.dtype == np.uint32 else np.nonzero(~np.isnan(exp))[0]
        idx, sc = bc.filter_many(op, corpus, score_cutoff=cutoff)
        assert idx.tolist() == some.tolist() and sc.tolist() == exp[some].tolist(), (op, cutoff)
        assert bc.last_filter_count == some.size
    # capacity overflow: the TRUE count comes back, and `capacity` valid pairs in ascending index order (rfgpu.h: not necessarily the first ones)
    exp = R.ops(N.OP_DISTANCE, qv, rows, lens, 30)
    some = np.nonzero(exp != R.NONE_U32)[0]
    assert some.size > 50
    idx, sc = bc.filter_many(N.OP_DISTANCE, corpus, score_cutoff=30, capacity=50)
    assert bc.last_filter_count == some.size and len(idx) == 50 and np.all(np.diff(idx.astype(np.int64)) > 0)
    assert np.isin(idx, some).all() and sc.tolist() == exp[idx.astype(np.int64)].tolist()


def test_many_multi_with_three_comparators():
    q, cands = _road_case(13, n=1500)
    corpus, rows, lens = _bytes_corpus(cands)
    rng = np.random.default_rng(14)
    qs = [q, _planted(rng, q, 62), _rand(rng, 70, 62)]
    bcs = [DL.BatchComparator(bytes(48 + v for v in x)) for x in qs]
    for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_DISTANCE, 12), (N.OP_NORMALIZED_SIMILARITY, 0.4)):
        got = DL.BatchComparator.many_multi(bcs, op, corpus, score_cutoff=cutoff)
        for j, x in enumerate(qs):
            _eq(got[j], R.ops(op, [48 + v for v in x], rows, lens, cutoff), f"many_multi row {j} op {op}")


def test_slot_order_and_stream_many(tmp_path):
    q, cands = _road_case(15)
    corpus, rows, lens = _bytes_corpus(cands)
    bc = DL.BatchComparator(bytes(48 + v for v in q))
    qv = [48 + v for v in q]
    slots = corpus.slot_index()
    real = np.nonzero(slots != 0xFFFFFFFF)[0]
    assert real.size == len(cands)
    for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_DISTANCE, 9), (N.OP_NORMALIZED_DISTANCE, None)):
        exp = R.ops(op, qv, rows, lens, cutoff)
        got = bc.many(op, corpus, rf.Args().slot_order(), score_cutoff=cutoff)
        assert got.size == corpus.slot_count
        _eq(got[real], exp[slots[real].astype(np.int64)], f"slot order op {op}")
    path = str(tmp_path / "dl.rfc")
    corpus.save(path)
    for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 20), (N.OP_NORMALIZED_SIMILARITY, 0.5)):
        _eq(bc.stream_many(op, path, score_cutoff=cutoff, segment_bytes=32768), R.ops(op, qv, rows, lens, cutoff), f"stream_many op {op}")


# ------------------------------------------------------------------------------------------------ pack-time layouts, each in a child process
CHILD = os.environ.get("RF_TEST_DL_CHILD") == "1"


@pytest.mark.parametrize("knob", ["RF_NO_MIXED_TILES", "RF_NO_RENAME"])
def test_pack_time_layouts(knob):
    if not CHILD:
        node = f"{os.path.abspath(__file__)}::test_pack_time_layouts[{knob}]"
        r = subprocess.run([sys.executable, "-m", "pytest", node, "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=ROOT,
                           env=dict(os.environ, RF_TEST_DL_CHILD="1", **{knob: "1"}), timeout=900)
        assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])  # one child, never retried
        return
    assert os.environ.get(knob) == "1"
    for qlen in (24, 64, 90):
        rng = np.random.default_rng(qlen)
        q = _rand(rng, qlen, 62)
        rows, plant = _shape_rows("bucketed", rng, q, 62)
        corpus, r, lens = _bytes_corpus(rows + plant)
        _parity(bytes(48 + v for v in q), corpus, r, lens, f"{knob} query {qlen}", ops=(N.OP_DISTANCE, N.OP_NORMALIZED_SIMILARITY))
        exp = R.ops(N.OP_DISTANCE, [48 + v for v in q], r, lens, 12)
        some = np.nonzero(exp != R.NONE_U32)[0]
        bc = DL.BatchComparator(bytes(48 + v for v in q))
        idx, sc = bc.filter_many(N.OP_DISTANCE, corpus, score_cutoff=12)
        assert idx.tolist() == some.tolist() and sc.tolist() == exp[some].tolist()
        scores, idx = bc.topk(corpus, 16)
        full = R.ops(N.OP_DISTANCE, [48 + v for v in q], r, lens)
        order = sorted(range(len(full)), key=lambda i: (full[i], i))[:16]
        assert idx.tolist() == order and scores.tolist() == full[order].tolist()


# ------------------------------------------------------------------------------------------------ randomized differential test
def test_randomized_corpus_models():
    """a few hundred seeds; symbol law, length law, op and cutoff drawn per seed"""
    for seed in range(240):
        rng = np.random.default_rng(90000 + seed)
        sym = int(rng.choice([2, 3, 4, 26, 62, 200]))
        qlen = int(rng.choice([rng.integers(0, 17), rng.integers(17, 65), rng.integers(65, 130), rng.integers(250, 300)], p=[0.35, 0.4, 0.2, 0.05]))
        max_len = int(rng.choice([8, 32, 64, 100, 260], p=[0.2, 0.3, 0.3, 0.15, 0.05]))
        law = int(rng.integers(3))
        n = int(rng.integers(1, 200))
        q = _rand(rng, qlen, sym)
        cands = []
        for _ in range(n):
            if rng.random() < 0.3:
                cands.append(_planted(rng, q, sym, clip=max_len))
            else:
                L = max_len if law == 0 else (int(rng.integers(0, max_len + 1)) if law == 1 else int(min(max_len, rng.geometric(0.08))))
                cands.append(_rand(rng, L, sym))
        base = 0 if sym == 200 else 48
        corpus, rows, lens = _bytes_corpus(cands, base=base)
        qb = bytes(base + v for v in q)
        op = int(rng.integers(4))
        cutoff = None if rng.random() < 0.3 else (float(rng.random()) if op >= 2 else int(rng.integers(0, max(qlen, max_len) + 3)))
        got = DL.BatchComparator(qb).many(op, corpus, score_cutoff=cutoff)
        _eq(got, R.ops(op, [base + v for v in q], rows, lens, cutoff), f"seed {seed}: sym {sym} query {qlen} max_len {max_len} law {law} n {n} op {op} cutoff {cutoff}")
