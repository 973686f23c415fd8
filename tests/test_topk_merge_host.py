"""The host side of the top-k exchange, no GPU involved: rf_topk_merge_entries and rf_topk_merge_u32 on synthetic lists (the entry vectors that
tests/test_gpu_topk_selection.py gives the device merge), and rf_topk_entry_score_u32 / rf_topk_entry_score_f64 against the key definitions of
include/rfgpu.h."""
import math
import struct

import numpy as np
import pytest

from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd import parallel

import topk_select_check as T


@pytest.mark.parametrize("n", T.ENTRY_NS)
def test_merge_entries_on_synthetic_entries(n):
    """shared keys, indices on both sides of 2^32, empties in between, k below, at and beyond n: a Python sort by (key, index), padded with empty entries"""
    for seed in (n, n + 1):
        e = T.synthetic_entries(n, 9000 + seed)
        for k in T.entry_ks(n):
            got = [tuple(r) for r in parallel.merge_entries(e, k).tolist()]
            assert got == T.expected_entries(e, k), (n, k)
    nothing = np.full((n, 2), T.U64MAX, dtype=np.uint64)
    assert parallel.merge_entries(nothing, 3).tolist() == [[T.EMPTY, T.EMPTY]] * 3


def _lists(rng, counts, k, hi_scores):
    """row-major [lists, k] scores and indices, row l valid up to counts[l]: scores from a handful of values (ties within and across lists), unique indices
    on both sides of 2^32; the rest of a row is garbage that must not be read as entries"""
    lists = len(counts)
    scores = rng.integers(0, 2**32, size=(lists, k), dtype=np.uint64).astype(np.uint32)
    indices = rng.integers(0, 2**63, size=(lists, k), dtype=np.uint64)
    values = [0, 1, 2, 7, 0xFFFFFFFE] if hi_scores else [0, 1, 2, 7]
    pool = np.concatenate([np.arange(0, 40), 2**32 - 20 + np.arange(0, 40), 2**40 + np.arange(0, 40)]).astype(np.uint64)
    assert sum(counts) <= len(pool)
    take = rng.permutation(pool)
    at = 0
    for l, c in enumerate(counts):
        scores[l, :c] = rng.choice(values, size=c)
        indices[l, :c] = take[at: at + c]
        at += c
    return scores, indices


@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
@pytest.mark.parametrize("counts", [(0,), (0, 0, 0), (5,), (16,), (0, 16, 3), (16, 16, 16), (1, 0, 15, 16, 2), (16, 0)])
def test_merge_topk_of_lists(op, counts):
    """rf_topk_merge_u32: lists whose counts are 0, below k and k; ties across lists broken by the index, indices beyond 2^32; ascending scores for the
    distance op, descending for the similarity op"""
    k = 16
    rng = np.random.default_rng(100 * len(counts) + sum(counts) + op)
    scores, indices = _lists(rng, counts, k, hi_scores=True)
    s, i = parallel.merge_topk(op, scores, indices, np.array(counts, dtype=np.uint32), k)
    pairs = [(int(scores[l, j]), int(indices[l, j])) for l, c in enumerate(counts) for j in range(c)]
    pairs.sort(key=lambda p: (-p[0] if op == N.OP_SIMILARITY else p[0], p[1]))
    assert list(zip(s.tolist(), i.tolist())) == pairs[:k]
    if sum(counts) > 16:  # (what the case is for)
        assert len({p[0] for p in pairs[:k]}) < len(pairs[:k]) and any(p[1] >= 2**32 for p in pairs[:k]) and any(p[1] < 2**32 for p in pairs[:k])


def test_merge_topk_breaks_a_tie_across_lists_by_index():
    k = 3
    scores = np.array([[5, 5, 9], [5, 5, 5]], dtype=np.uint32)
    indices = np.array([[2**32 + 1, 2**32 + 7, 0], [3, 2**32 + 2, 2**33]], dtype=np.uint64)
    for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        s, i = parallel.merge_topk(op, scores, indices, np.array([2, 3], dtype=np.uint32), k)
        assert s.tolist() == [5, 5, 5] and i.tolist() == [3, 2**32 + 1, 2**32 + 2]
    s, i = parallel.merge_topk(N.OP_SIMILARITY, scores, indices, np.array([3, 3], dtype=np.uint32), k)
    assert s.tolist() == [9, 5, 5] and i.tolist() == [0, 3, 2**32 + 1]


def test_entry_score_u32_inverts_the_key_definition():
    """rfgpu.h: the key of a u32 score is the score (RF_OP_DISTANCE) or 0xFFFFFFFF - score (RF_OP_SIMILARITY)"""
    L = N.lib()
    for score in (0, 1, 64, 2047, 2048, 2**22, 4_800_000, 2**31, 0xFFFFFFFE):
        assert L.rf_topk_entry_score_u32(score, 0) == score
        assert L.rf_topk_entry_score_u32(0xFFFFFFFF - score, 1) == score
    assert parallel.decode_entries(np.array([[3, 2**40], [T.EMPTY, T.EMPTY], [0xFFFFFFFF - 3, 7]], dtype=np.uint64), N.OP_SIMILARITY, False) == [(0xFFFFFFFC, 2**40), (3, 7)]


def _f64_key(x, descending):
    """rfgpu.h: the IEEE bits with the sign bit flipped (negative values: all bits flipped), complemented for the descending ops"""
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    b = (b ^ 0xFFFFFFFFFFFFFFFF) if b >> 63 else (b ^ 0x8000000000000000)
    return (b ^ 0xFFFFFFFFFFFFFFFF) if descending else b


def test_entry_score_f64_inverts_the_key_definition():
    """at 0.0, -0.0, 1.0 and the doubles next to each of them: the score comes back bit for bit, and the keys order as the scores do"""
    L = N.lib()
    xs = []
    for x in (0.0, -0.0, 1.0):
        xs += [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]
    xs += [-1.0, 0.5, 0.9999999999999999, 1e-300, 1.7976931348623157e308, -1.7976931348623157e308]
    for desc in (0, 1):
        for x in xs:
            got = L.rf_topk_entry_score_f64(_f64_key(x, desc), desc)
            assert struct.pack("<d", got) == struct.pack("<d", x), (x, desc, got)
        # smaller key = better: ascending scores for the distance ops, descending for the similarity ops; -0.0 sorts directly below 0.0
        order = sorted({struct.pack("<d", x): x for x in xs}.values(), key=lambda x: (x, math.copysign(1.0, x)))  # (each bit pattern once)
        keys = [_f64_key(x, desc) for x in order]
        assert keys == sorted(set(keys), reverse=bool(desc)), desc
    assert _f64_key(0.0, 0) == 0x8000000000000000 and _f64_key(-0.0, 0) == 0x7FFFFFFFFFFFFFFF and _f64_key(1.0, 0) == 0xBFF0000000000000
    assert _f64_key(1.0, 1) == 0x400FFFFFFFFFFFFF  # (the best normalized similarity: a key with bit 63 clear, an index_base beyond 2^32 beside it)
    got = parallel.decode_entries(np.array([[_f64_key(1.0, 1), 2**33], [_f64_key(0.0, 1), 1], [T.EMPTY, T.EMPTY]], dtype=np.uint64), N.OP_NORMALIZED_SIMILARITY, True)
    assert got == [(1.0, 2**33), (0.0, 1)]
