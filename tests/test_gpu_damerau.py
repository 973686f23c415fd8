"""damerau_levenshtein::BatchComparator on the device (rf_damerau.hip), bit-exact against tests/dl_reference.py: the reference's known answers,
parity over corpus shapes x query lengths x ops x cutoffs (the register kernels, the LDS rows with 8- and 16-bit fields, the global rows), every
result road, two pack-time layouts through child processes, and a randomized differential test.
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
