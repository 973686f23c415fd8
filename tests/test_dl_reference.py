"""tests/dl_reference.py is what the device's Damerau-Levenshtein results are held to (tests/test_gpu_damerau.py), so it is held here first: the
vectorised form against an independent full-matrix implementation, the reference's own known answers (damerau_levenshtein.rs tests), and the
metric's place among its neighbours (DL <= OSA <= Levenshtein, symmetry, triangle inequality).  Also the host-only part of the new surface:
the Python module and constant, and the C ABI's comparator calls, accept the metric.  No GPU."""
import ctypes as C
import random

import numpy as np
import pytest

import dl_reference as R
import textbook

KNOWN = [("", "", 0), ("aaaa", "", 4), ("aaaa", "aaaa", 0), ("aaaa", "aaa", 1), ("aaaa", "aaab", 1), ("abaa", "baaa", 1), ("aaaa", "bbbb", 4), ("CA", "ABC", 2)]
KNOWN_NORM_SIM = [1.0, 0.75, 0.75, 0.75, 0.0]  # normalized_similarity at score_cutoff 0.0 of KNOWN[2:7]
KNOWN_CHARS = [("Иванко", "Петрунко", 5), ("ИвaнкoIvan", "Петрунко", 10)]


def _codes(s):
    return [ord(c) for c in s]


def _many_one(a, b):
    rows, lens = R.pad_rows([_codes(b)])
    return int(R.dl_many(_codes(a), rows, lens)[0])


def test_known_answers():
    for a, b, d in KNOWN:
        assert R.dl_pair(a, b) == d and _many_one(a, b) == d and _many_one(b, a) == d, (a, b)
    for (a, b, d), ns in zip(KNOWN[2:7], KNOWN_NORM_SIM):
        assert R.op_pair(R.OP_NORMALIZED_SIMILARITY, d, len(a), len(b), 0.0) == ns, (a, b)
    for a, b, d in KNOWN_CHARS:
        assert R.dl_pair(a, b) == d and _many_one(a, b) == d, (a, b)
    assert textbook.osa("CA", "ABC") == 3  # the neighbour that is not a metric


@pytest.mark.parametrize("sym", [2, 4, 62])
def test_vectorised_form_equals_the_full_matrix(sym):
    rng = random.Random(1000 + sym)
    total = 0
    for _ in range(12):
        q = [rng.randrange(sym) for _ in range(rng.randint(0, 80))]
        cands = [[rng.randrange(sym) for _ in range(rng.randint(0, 80))] for _ in range(100)]
        rows, lens = R.pad_rows(cands)
        got = R.dl_many(q, rows, lens)
        assert got.tolist() == [R.dl_pair(q, c) for c in cands]
        total += len(cands)
    assert total >= 1000  # x 3 alphabets: a few thousand pairs


def test_order_among_the_neighbours_symmetry_and_triangle():
    rng = random.Random(77)
    for sym in (3, 4, 62):
        strs = [[rng.randrange(sym) for _ in range(rng.randint(0, 24))] for _ in range(40)]
        d = [[R.dl_pair(a, b) for b in strs] for a in strs]
        for i, a in enumerate(strs):
            for j, b in enumerate(strs):
                assert d[i][j] == d[j][i]
                assert d[i][j] <= textbook.osa(a, b) <= textbook.levenshtein(a, b)
        n = len(strs)
        for _ in range(4000):
            i, j, k = rng.randrange(n), rng.randrange(n), rng.randrange(n)
            assert d[i][k] <= d[i][j] + d[j][k]


def test_ops_under_cutoffs():
    # "aaaa" / "aaab": d = 1, maximum = 4
    assert R.op_pair(R.OP_DISTANCE, 1, 4, 4, 1) == 1 and R.op_pair(R.OP_DISTANCE, 1, 4, 4, 0) is None
    assert R.op_pair(R.OP_SIMILARITY, 1, 4, 4, 3) == 3 and R.op_pair(R.OP_SIMILARITY, 1, 4, 4, 4) is None
    assert R.op_pair(R.OP_SIMILARITY, 1, 4, 4, 9) is None  # cutoff above the maximum
    assert R.op_pair(R.OP_NORMALIZED_DISTANCE, 1, 4, 4, 0.25) == 0.25 and R.op_pair(R.OP_NORMALIZED_DISTANCE, 1, 4, 4, 0.2) is None
    assert R.op_pair(R.OP_NORMALIZED_SIMILARITY, 1, 4, 4, 0.75) == 0.75 and R.op_pair(R.OP_NORMALIZED_SIMILARITY, 1, 4, 4, 0.8) is None
    # cutoff below |len1 - len2|: the reference's _distance answers usize::MAX; distance -> None, similarity -> None (the deliberate difference)
    assert R.op_pair(R.OP_DISTANCE, 4, 4, 0, 3) is None and R.op_pair(R.OP_SIMILARITY, 4, 4, 0, 1) is None
    assert R.op_pair(R.OP_SIMILARITY, 4, 4, 0, 0) == 0
    out = R.ops(R.OP_DISTANCE, b"aaaa", *R.pad_rows([b"aaab", b"", b"bbbb"]), cutoff=1)
    assert out.dtype == np.uint32 and out.tolist() == [1, R.NONE_U32, R.NONE_U32]
    out = R.ops(R.OP_NORMALIZED_SIMILARITY, b"aaaa", *R.pad_rows([b"aaab", b"", b"bbbb"]), cutoff=0.5)
    assert out[0] == 0.75 and np.isnan(out[1]) and np.isnan(out[2])


def test_the_metric_is_offered_on_the_host_side():
    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N

    assert rf.N.DAMERAU_LEVENSHTEIN == 7 and "damerau_levenshtein" in rf.distance.__all__
    mod = rf.distance.damerau_levenshtein
    assert mod.BatchComparator.METRIC == 7 and not mod.BatchComparator.FLOAT
    L = N.lib()
    for q in (b"", b"CA", bytes(range(200)) * 2, "Иванко"):
        bc = mod.BatchComparator(q)
        assert L.rf_comparator_metric(bc._h) == N.DAMERAU_LEVENSHTEIN and L.rf_comparator_query_len(bc._h) == len(q)
        cl = bc.clone()
        assert L.rf_comparator_metric(cl._h) == N.DAMERAU_LEVENSHTEIN and L.rf_comparator_query_len(cl._h) == len(q)
        del cl, bc
    # the first value past the metric range is still refused
    h = C.c_void_p()
    buf = (C.c_uint8 * 1)(0)
    assert L.rf_comparator_new(8, buf, 1, C.byref(h)) == N.RF_ERR_INVALID_ARG
