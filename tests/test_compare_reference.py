"""tests/compare_reference.py is what the device's hamming / prefix / postfix results are held to (tests/test_gpu_compare.py), so it is held here
first: the reference's own known answers (tests/golden/compare_known_answers.json, extracted from its test modules and doc examples), the
vectorised form against the plain loops, postfix as prefix of the reversed strings, and two pins to the oracle that fix what the four ops do with
and without score_cutoff -- on pairs where a metric the oracle knows has the same value by construction.  No GPU."""
import json
import math
import os
import random

import numpy as np
import pytest

import compare_reference as R
from oracle import oracle as o
from rapidfuzz_rs_amd import _native as N

# the restatement speaks the product's encodings and op numbers: what the GPU tests compare by bits
assert (R.NONE_U32, R.DIFFERENT_LENGTH_U32, R.NONE_F64_BITS, R.DIFFERENT_LENGTH_F64_BITS) == (N.NONE_U32, N.DIFFERENT_LENGTH_U32, N.NONE_F64_BITS, N.DIFFERENT_LENGTH_F64_BITS)
assert (R.OP_DISTANCE, R.OP_SIMILARITY, R.OP_NORMALIZED_DISTANCE, R.OP_NORMALIZED_SIMILARITY) == (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "compare_known_answers.json"), encoding="utf-8"))
OPS = {"distance": R.OP_DISTANCE, "similarity": R.OP_SIMILARITY}
ALL_OPS = (R.OP_DISTANCE, R.OP_SIMILARITY, R.OP_NORMALIZED_DISTANCE, R.OP_NORMALIZED_SIMILARITY)


def test_the_fixture_holds_the_references_cases():
    assert len(KNOWN) >= 20 and {e["metric"] for e in KNOWN} == set(R.METRICS)
    diff = [e for e in KNOWN if e["s1"] == "hammers" and e["s2"] == "hamming"]
    assert sorted((e["pad"] is True, e["cutoff"], e["expect"]) for e in diff if e["cutoff"]) == [(False, 2, None), (False, 3, 3), (True, 2, None), (True, 3, 3)]
    assert any(e["s2"] == "h香mmüng" and e["expect"] == 2 for e in KNOWN)
    assert any(e["expect"] == "DifferentLengthArgs" for e in KNOWN)


@pytest.mark.parametrize("e", KNOWN, ids=[f"{e['source']}" for e in KNOWN])
def test_known_answers(e):
    a, b = e["s1"], e["s2"]
    raw = R.pair(e["metric"], a, b)
    got = R.op_pair(e["metric"], OPS[e["op"]], raw, len(a), len(b), e["cutoff"], bool(e["pad"]))
    exp = R.ERR if e["expect"] == "DifferentLengthArgs" else e["expect"]
    assert got is exp or got == exp, (e, got)
    # ... and through the vectorised form
    rows, lens = R.pad_rows([R._codes(b)])
    assert int(R.raw_many(e["metric"], a, rows, lens)[0]) == raw


@pytest.mark.parametrize("sym", [1, 2, 4, 62])
def test_vectorised_form_equals_the_loops_and_postfix_is_prefix_reversed(sym):
    rng = random.Random(500 + sym)
    for _ in range(10):
        q = [rng.randrange(sym) for _ in range(rng.randint(0, 70))]
        cands = [[rng.randrange(sym) for _ in range(rng.randint(0, 70))] for _ in range(120)]
        cands += [q[:k] + [sym + 1] * (k % 3) for k in range(0, len(q) + 1, 5)] + [q[k:] for k in range(0, len(q) + 1, 7)] + [q, q + q[:3], q[::-1]]
        rows, lens = R.pad_rows(cands)
        for metric in R.METRICS:
            assert R.raw_many(metric, q, rows, lens).tolist() == [R.pair(metric, q, c) for c in cands], metric
        assert [R.pair("postfix", q, c) for c in cands] == [R.pair("prefix", q[::-1], c[::-1]) for c in cands]
        rrows, rlens = R.pad_rows([c[::-1] for c in cands])
        assert R.raw_many("postfix", q, rows, lens).tolist() == R.raw_many("prefix", q[::-1], rrows, rlens).tolist()


def _cutoffs(op, values, maximum):
    """no cutoff; an attained value and one on either side of it; and the far ends"""
    if op in (R.OP_DISTANCE, R.OP_SIMILARITY):
        cs = {0, 1, maximum, maximum + 1, maximum + 7}
        for v in values:
            cs |= {max(v - 1, 0), v, v + 1}
        return [None] + sorted(cs)
    cs = {0.0, 0.5, 1.0}
    for v in values:
        cs |= {v, math.nextafter(v, 0.0), math.nextafter(v, 2.0)}
    return [None] + sorted(c for c in cs if 0.0 <= c <= 1.0)


def _oracle_value(mod, op, q, c, cutoff):
    if op == R.OP_SIMILARITY and cutoff is not None and mod is o.levenshtein:
        # (the reference's Levenshtein similarity above its cutoff is a wrapped `maximum - usize::MAX`, details/distance.rs:209-210 -- the deliberate difference
        # Q2 of include/rfgpu.h; hamming's own _distance never answers usize::MAX, so its similarity is the uncut value kept where it reaches the cutoff)
        v = mod._call(op, q, c)
        return v if v >= cutoff else None
    return mod._call(op, q, c, score_cutoff=cutoff)


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a == b)


def test_prefix_is_pinned_to_the_oracles_lcs_seq():
    """candidate = query[:p] + symbols the query does not hold: every common subsequence lies in query[:p], so LCS = p = the common prefix, and lcs_seq has
    prefix's maximum and prefix's MetricUsize defaults -- every op, every cutoff must agree (postfix: the mirror image)"""
    rng = random.Random(11)
    checked = 0
    for len1 in (1, 7, 16, 33, 64):
        q = bytes(rng.randrange(97, 110) for _ in range(len1))
        for p in sorted({0, 1, len1 // 2, len1 - 1, len1}):
            for tail in (0, 1, 5, len1 + 3):
                c = q[:p] + bytes(rng.randrange(48, 58) for _ in range(tail))
                cm = bytes(reversed(c))
                qm = bytes(reversed(q))
                assert R.pair("prefix", q, c) == p and R.pair("postfix", qm, cm) == p
                maximum = max(len1, len(c))
                for op in ALL_OPS:
                    uncut = R.op_pair("prefix", op, p, len1, len(c))
                    for cutoff in _cutoffs(op, [uncut], maximum):
                        exp = _oracle_value(o.lcs_seq, op, q, c, cutoff)
                        assert _same(R.op_pair("prefix", op, p, len1, len(c), cutoff), exp), ("prefix", op, q, c, cutoff, exp)
                        assert _same(R.op_pair("postfix", op, p, len1, len(c), cutoff), exp), ("postfix", op, q, c, cutoff, exp)
                        checked += 1
    assert checked > 2000


def test_hamming_is_pinned_to_the_oracles_levenshtein():
    """candidate = the query with k positions replaced by symbols the query does not hold: each of them costs one edit whatever the alignment, so the
    Levenshtein distance is k = the Hamming distance, and Levenshtein at unit weights has hamming's maximum and hamming's MetricUsize defaults"""
    rng = random.Random(12)
    checked = 0
    for len1 in (1, 7, 16, 33, 64):
        q = bytes(rng.randrange(97, 110) for _ in range(len1))
        for k in sorted({0, 1, len1 // 3, len1 - 1, len1}):
            c = bytearray(q)
            for pos in rng.sample(range(len1), k):
                c[pos] = rng.randrange(48, 58)
            c = bytes(c)
            assert R.pair("hamming", q, c) == k
            for op in ALL_OPS:
                uncut = R.op_pair("hamming", op, k, len1, len1)
                for cutoff in _cutoffs(op, [uncut], len1):
                    exp = _oracle_value(o.levenshtein, op, q, c, cutoff)
                    for pad in (False, True):  # equal lengths: pad changes nothing
                        assert _same(R.op_pair("hamming", op, k, len1, len1, cutoff, pad), exp), (op, q, c, cutoff, pad, exp)
                    checked += 1
    assert checked > 400


def test_hamming_lengths_and_pad():
    assert R.op_pair("hamming", R.OP_DISTANCE, R.pair("hamming", "ham", "hamming"), 3, 7) is R.ERR
    assert R.op_pair("hamming", R.OP_NORMALIZED_SIMILARITY, 4, 3, 7, 0.5) is R.ERR  # before any cutoff
    assert R.op_pair("hamming", R.OP_DISTANCE, 4, 3, 7, None, True) == 4 and R.op_pair("hamming", R.OP_DISTANCE, 4, 3, 7, 3, True) is None
    assert R.op_pair("hamming", R.OP_SIMILARITY, 4, 3, 7, None, True) == 3 and R.op_pair("hamming", R.OP_SIMILARITY, 4, 3, 7, 9, True) is None
    rows, lens = R.pad_rows([b"hamming", b"ham", b"", b"humming"])
    out = R.ops("hamming", R.OP_DISTANCE, b"hamming", rows, lens, cutoff=0)
    assert out.dtype == np.uint32 and out.tolist() == [0, R.DIFFERENT_LENGTH_U32, R.DIFFERENT_LENGTH_U32, R.NONE_U32] and R.keep(out).tolist() == [0]
    out = R.ops("hamming", R.OP_NORMALIZED_DISTANCE, b"hamming", rows, lens, cutoff=0.0)
    assert out.view(np.uint64).tolist() == [0, R.DIFFERENT_LENGTH_F64_BITS, R.DIFFERENT_LENGTH_F64_BITS, R.NONE_F64_BITS] and np.isnan(out[1:]).all()
    assert R.keep(out).tolist() == [0]
    out = R.ops("hamming", R.OP_DISTANCE, b"hamming", rows, lens, pad=True)
    assert out.tolist() == [0, 4, 7, 1]
