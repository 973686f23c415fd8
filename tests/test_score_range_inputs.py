"""The corpora of tests/score_range_inputs.py reach what tests/test_gpu_score_range.py needs them for (no GPU: the CPU oracle).

The GPU legs compare u32 scores at and above 2^31 with the oracle.  A change to a generator could quietly drop every value below 2^31, or every one above it,
or the values between the cutoffs, and the GPU legs would stay green for the wrong reason.  So the conditions are asserted here from the oracle's values:
bounds rather than exact literals, except where a literal is the point."""
import numpy as np
import pytest

import score_range_inputs as S
import topk_select_check as T
from rapidfuzz_rs_amd import _native as N


def _lengths(offsets):
    return np.diff(offsets.astype(np.int64))


def _kept(name, weights, op, cutoff):
    return int((S.scores(name, weights, op, cutoff) != T.U64MAX).sum())


def _straddles(name, weights, n):
    """the conditions of a ragged corpus: both sides of 2^31 well filled, bit 31 the first digit that differs, many distinct values, cutoffs that split"""
    d = S.scores(name, weights, N.OP_DISTANCE)
    assert len(d) == n and (d != T.U64MAX).all()
    above, below = int((d >= S.BIT31).sum()), int((d < S.BIT31).sum())
    assert above >= 40 and below >= 40, (above, below)
    assert T.highest_bit(int(d.min()) ^ int(d.max())) == 31
    assert len(np.unique(d)) >= 100
    assert int(d.max()) <= S.TOP
    median = S.median_cutoff(name, weights)
    assert median >= S.BIT31  # more than half of the scores have bit 31 set: the median cutoff itself has
    for cutoff in (median, S.BIT31 - 1, S.BIT31):
        kept = _kept(name, weights, N.OP_DISTANCE, cutoff)
        assert kept == int((d <= cutoff).sum())  # (the oracle under a cutoff is its uncut result, thresholded)
        assert 4 * kept >= n and 4 * (n - kept) >= n, (cutoff, kept)
    assert _kept(name, weights, N.OP_DISTANCE, S.BIT31 - 1) == _kept(name, weights, N.OP_DISTANCE, S.BIT31) == below  # no distance is 2^31 itself
    for cutoff in (S.TOP, 0xFFFFFFFF, 2**32, 2**40):
        assert _kept(name, weights, N.OP_DISTANCE, cutoff) == n
    assert 1 <= _kept(name, weights, N.OP_DISTANCE, 3 * S.factor(weights)) <= 3  # the tight cutoff keeps the edited copies of the query only
    assert _kept(name, weights, N.OP_DISTANCE, 0) == 0
    return d


def test_uniform_ragged_straddles_bit_31():
    q, data, offsets = S.uniform_ragged()
    lens = _lengths(offsets)
    assert len(q) == 48 and len(lens) == 201 and int(lens.max()) == S.UNIFORM_MAX_LEN and int((lens == S.UNIFORM_MAX_LEN).sum()) >= 70
    assert {0, 1, 47, 48, 49, 32_767, 32_768, 32_769, 32_815, 32_816, 32_817} <= set(lens.tolist())
    assert 8_000_000 <= len(data) <= 9_500_000 and set(np.unique(data).tolist()) <= set(T.synth.ALNUM.tolist())
    assert 65535 * (48 + int(lens.max())) == 0xFFFF0000 <= S.TOP
    d = _straddles("uniform_ragged", S.W_UNIFORM, 201)
    assert int(d.max()) == 65535 * (S.UNIFORM_MAX_LEN - 48) == 0xFF9F0060  # a literal: the query is a subsequence of every longest candidate
    assert (d % 65535 == 0).all()
    # the similarity f x (Mx - lev) <= f x min(len1, len2) stays far below 2^31: say so
    s = S.scores("uniform_ragged", S.W_UNIFORM, N.OP_SIMILARITY)
    assert int(s.max()) == 48 * 65535 and int((s > 0).sum()) >= 150
    assert S.median_cutoff("uniform_ragged", S.W_UNIFORM, N.OP_SIMILARITY) > 1


def test_uniform_single_length_lies_above_bit_31():
    q, data, offsets = S.uniform_single_length()
    lens = _lengths(offsets)
    assert q == S.uniform_ragged()[0] and len(lens) == 200 and (lens == 40_000).all()
    assert 65535 * (48 + 40_000) <= S.TOP
    d = S.scores("uniform_single_length", S.W_UNIFORM, N.OP_DISTANCE)
    assert int(d.min()) >= 39_952 * 65535 > S.BIT31 and int(d.max()) <= S.TOP
    assert len(np.unique(d)) >= 3
    median = S.median_cutoff("uniform_single_length", S.W_UNIFORM)
    kept = _kept("uniform_single_length", S.W_UNIFORM, N.OP_DISTANCE, median)
    assert 50 <= kept <= 150  # the candidates that hold every symbol of the query sit at the minimum: the median cutoff splits
    assert _kept("uniform_single_length", S.W_UNIFORM, N.OP_DISTANCE, S.BIT31) == 0 and _kept("uniform_single_length", S.W_UNIFORM, N.OP_DISTANCE, S.TOP) == 200


@pytest.mark.parametrize("weights", [S.W_INDEL_EVEN, S.W_INDEL_ODD], ids=["sub65534", "sub65535"])
def test_indel_like_ragged_straddles_bit_31(weights):
    q, data, offsets = S.indel_like_ragged()
    lens = _lengths(offsets)
    assert len(q) == 48 and len(lens) == 199 and int(lens.max()) == S.INDEL_MAX_LEN and int((lens == S.INDEL_MAX_LEN).sum()) >= 70
    assert {0, 1, 48, 65_487, 65_488, 65_489, 65_490, 65_535, 65_536} <= set(lens.tolist())
    assert int((lens > 65_535).sum()) >= 40 and int((lens <= 65_535).sum()) >= 40  # both sides of the device packer's limit
    assert 16_000_000 <= len(data) <= 18_500_000
    assert 32767 * (48 + int(lens.max())) == 0xFFFF7FFD <= S.TOP
    d = _straddles("indel_like_ragged", weights, 199)
    assert int(d.max()) <= 32767 * (48 + S.INDEL_MAX_LEN) and int(d.max()) >= 0xFFC00000 and (d % 32767 == 0).all()
    # both tables finish as f x indel: the same values
    assert (d == S.scores("indel_like_ragged", S.W_INDEL_EVEN, N.OP_DISTANCE)).all()
    s = S.scores("indel_like_ragged", weights, N.OP_SIMILARITY)
    assert int(s.max()) == 2 * 32767 * 48 and int((s > 0).sum()) >= 150


def test_long_query_similarities_reach_bit_31():
    q, data, offsets = S.long_query()
    lens = _lengths(offsets)
    assert len(q) == S.LONG_QLEN and len(lens) == 44 and lens[-4:].tolist() == [S.LONG_QLEN, 20_000, 64, 0]
    assert 32767 * (len(q) + int(lens.max())) <= S.TOP
    s = S.scores("long_query", S.W_INDEL_EVEN, N.OP_SIMILARITY)
    assert int(s[0]) == 2 * 32767 * S.LONG_QLEN == int(s.max()) and int(s.max()) >= 0x80E00000  # the verbatim copy: lcs = 33 000
    above = int((s >= S.BIT31).sum())
    assert above >= 30 and len(s) - above >= 4 and int(s.min()) == 0, above  # the near-duplicates against the random strings and the ones with many edits
    assert len(np.unique(s)) >= 35
    assert T.highest_bit(int(s.min()) ^ int(s.max())) == 31
    assert _kept("long_query", S.W_INDEL_EVEN, N.OP_SIMILARITY, S.BIT31) == above
    d = S.scores("long_query", S.W_INDEL_EVEN, N.OP_DISTANCE)
    assert S.BIT31 > int(d.max()) >= 2**30 and int(d.min()) == 0  # the distances stay below bit 31 here: the similarity is what this corpus is for
    # the descending key 0xFFFFFFFE - s of the best entries has bit 31 CLEAR, that of the worst has it set
    ev, ei = T.select(s, 44, True, False)
    assert int(ev[0]) >= S.BIT31 > int(ev[-1]) and int(ei[0]) == 0


def test_general_boundary_is_the_last_accepted_worst_case():
    q, data, offsets = S.general_boundary()
    lens = _lengths(offsets)
    assert len(q) == 40 and len(lens) == 150 and int(lens.max()) == 32_768 - 40
    worst = (len(q) + int(lens.max())) * max(S.W_GENERAL)
    assert worst == S.BIT31 - 32_768 < S.BIT31 <= (len(q) + int(lens.max()) + 1) * max(S.W_GENERAL)
    d = S.scores("general_boundary", S.W_GENERAL, N.OP_DISTANCE)
    assert int(d.max()) >= 2**30 and int(d.max()) < S.BIT31 and len(np.unique(d)) >= 100
    median = S.median_cutoff("general_boundary", S.W_GENERAL)
    kept = _kept("general_boundary", S.W_GENERAL, N.OP_DISTANCE, median)
    assert 4 * kept >= 150 and 4 * (150 - kept) >= 150


def test_every_family_is_within_the_refusal_rule():
    """f x (len1 + max_len) <= 0xFFFFFFFE for every (corpus, weights, query) the GPU legs call, the second queries of the fused calls included"""
    for name, weights in S.SHORT_FAMILIES + (("long_query", S.W_INDEL_EVEN),):
        q, data, offsets = S.CORPORA[name]()
        assert S.factor(weights) * (len(q) + int(_lengths(offsets).max())) <= S.TOP, (name, weights)
        assert len(S.second_query(name)) <= len(q) or name == "long_query"


def test_cutoff_lists_hold_the_values_of_the_issue():
    for name, weights in S.SHORT_FAMILIES:
        cuts = S.distance_cutoffs(name, weights)
        assert set(cuts) >= {2**31 - 1, 2**31, 0xFFFFFFFE, 0xFFFFFFFF, 2**32, 2**40, 0, 3 * weights[0]} and len(set(cuts)) == 9
        assert S.BIT31 <= cuts[0] <= S.TOP
        sims = S.similarity_cutoffs(name, weights)
        assert set(sims) >= {0, 1, 2**31, 0xFFFFFFFF, 2**32} and 1 < sims[2] < S.BIT31
