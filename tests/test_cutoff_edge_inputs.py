"""The inputs of tests/test_gpu_cutoff_edges.py held to their conditions on the host (no GPU; a few seconds): tests/cutoff_edge_inputs.py builds them.

These are conditions, not measurements.  What the oracle showed when this was written, summed over the grid of each leg (ragged alphanumeric corpus, 5-symbol query,
3037 candidates; candidates whose answer under the cutoff differs from the uncut value filtered by the compare):
    distance legs    Jaro 12, Jaro-Winkler prefix_weight 0.0: 12, 0.1: 17, 0.25: 23, 0.3: 16 (normalized_distance: the same counts)
    similarity legs  Jaro 0, Jaro-Winkler 0.1: 1, 0.25: 8, 0.3: 7 (normalized_similarity: 0 everywhere)
    over the alphabet `abcd` the distance legs show none and the similarity legs 3 (0.1) and 4 (0.25)
Triples that cutoff_grid() dropped because their two neighbours keep the same number of candidates: one each in the distance legs of Jaro-Winkler 0.1 and 0.25,
two in those of 0.3 and one in its similarity leg; none in any leg of a usize metric."""
import numpy as np
import pytest

import cutoff_edge_inputs as I

ND, NS = I.OP_NORMALIZED_DISTANCE, I.OP_NORMALIZED_SIMILARITY


@pytest.fixture(scope="module")
def alnum5():
    data, offsets, q = I.ragged("alnum", 5)
    return ("ragged", data, offsets), q


def _flips(corpus, q, name, op):
    scorer = I.Scorer(I.BY_NAME[name], q, corpus)
    cutoffs, _, _ = I.cutoff_grid(scorer, op)
    return I.flips(scorer, op, cutoffs)


@pytest.mark.parametrize("name", ["jaro", "jaro_winkler(0.0)", "jaro_winkler(0.1)", "jaro_winkler(0.25)", "jaro_winkler(0.3)"])
@pytest.mark.parametrize("op", [I.OP_DISTANCE, ND])
def test_distance_legs_of_the_5_symbol_query_hold_answers_no_filtered_uncut_value_gives(alnum5, name, op):
    """a device that computed the right score and filtered it with the plain compare would be wrong on these candidates"""
    found = _flips(*alnum5, name, op)
    print(name, I.OP_NAMES[op], len(found), found[:3])
    assert len(found) > 0


def test_similarity_leg_of_jaro_winkler_025_holds_one_too(alnum5):
    found = _flips(*alnum5, "jaro_winkler(0.25)", I.OP_SIMILARITY)
    print(len(found), found[:3])
    assert len(found) > 0


def _grids(legs):
    for leg in legs:
        for case in I.multitile_cases(2) if leg == "multitile" else I.leg_cases(leg):
            for metric in case.metrics:
                scorer = I.Scorer(metric, case.q, case.corpus)
                for op in metric.ops:
                    yield leg, case, metric, op, scorer, I.cutoff_grid(scorer, op, case.extra(metric, op), case.most)


@pytest.mark.parametrize("legs", [("lev-alnum", "lcs-alnum"), ("lev-abcd", "lcs-abcd"), ("jaro-alnum",), ("jaro-abcd",), ("rows-lev", "rows-lcs", "table-edge"), ("rows-jaro",),
                                  ("jaro-multiword", "chars", "multitile")], ids=lambda legs: "+".join(legs))
def test_every_triple_can_tell_a_flipped_compare(legs):
    """for every picked v with both neighbours inside [0, 1] the oracle keeps a different number of candidates at prev(v) and at next(v); the grid holds the
    triple of every kept v, then the fixed cutoffs, and nothing else.  Every leg of the GPU file is visited (the -few and -64 legs are subsets of these); the
    usize metrics never lose a triple, a Jaro / Jaro-Winkler leg two at the most (prefix_weight 0.3, 5-symbol query)"""
    triples = 0
    for leg, case, metric, op, scorer, (cutoffs, kept, dropped) in _grids(legs):
        assert len(kept) + len(dropped) <= case.most and len(kept) >= 2, (leg, case.tag, metric, op, kept, dropped)
        assert cutoffs[3 * len(kept):] == list(I.FIXED)
        full = scorer(op)
        values = set(full[~np.isnan(full)].tolist())
        for j, v in enumerate(kept):
            assert v in values and cutoffs[3 * j:3 * j + 3] == [I.prev(v), v, I.next_(v)]
            if I.prev(v) >= 0.0 and I.next_(v) <= 1.0:
                assert I.somes(scorer(op, I.prev(v))) != I.somes(scorer(op, I.next_(v))), (leg, case.tag, metric, op, v)
                triples += 1
        if metric.family != "jaro":
            assert not dropped, (leg, case.tag, metric, op, dropped)
        assert len(dropped) <= 2
    assert triples > 0


def test_grid_holds_the_planning_thresholds_and_the_quotients():
    """the smallest and the largest value, the value nearest each planning threshold, and for Levenshtein / OSA with a 64-symbol query over 64-symbol rows the
    quotients k / maximum, k = 2..5 (where plan_band_filter's K crosses 3): all of them produced by the corpus, all of them in the grid"""
    case = next(iter(I.leg_cases("rows-lev64")))
    assert case.len2 == 64 and len(case.q) == 64
    for metric in case.metrics:
        scorer = I.Scorer(metric, case.q, case.corpus)
        for op in metric.ops:
            _, kept, _ = I.cutoff_grid(scorer, op, case.extra(metric, op), case.most)
            full = scorer(op)
            vals = np.unique(full[~np.isnan(full)])
            assert vals[0] in kept and vals[-1] in kept
            for mark in I.thresholds(metric, op):
                assert vals[np.argmin(np.abs(vals - mark))] in kept, (metric, op, mark)
            if metric.name != "levenshtein(2,2,3)":
                quotients = case.extra(metric, op)
                assert len(quotients) == 4 and all(x in kept for x in quotients), (metric, op, quotients, kept)
    assert I.thresholds(I.BY_NAME["jaro"], I.OP_DISTANCE) == [1.0 - 0.7, 1.0 - 0.6] and I.thresholds(I.BY_NAME["jaro"], I.OP_SIMILARITY) == [0.7, 0.6]
    assert I.thresholds(I.BY_NAME["indel"], ND) == [0.7, 0.4] and I.thresholds(I.BY_NAME["indel"], NS) == [1.0 - 0.7, 1.0 - 0.4]


def test_maximum_is_the_oracles():
    """maximum() here is the divisor of the oracle's normalized distance, for every usize metric of the legs"""
    for metric in [m for m in I.METRICS if m.family != "jaro" and m.module != "ratio"] + [I.indel_like(5)]:
        for qlen in (5, 33, 64):
            data, offsets, q = I.ragged("alnum", qlen, n=401)
            scorer = I.Scorer(metric, q, ("ragged", data, offsets))
            dist = scorer.batch.many(I.OP_DISTANCE, data, offsets, **metric.kw).astype(np.float64)
            mx = np.array([I.maximum(metric, qlen, int(n)) for n in np.diff(offsets).astype(np.int64)], dtype=np.float64)
            assert I.same(np.where(mx > 0, dist / np.where(mx > 0, mx, 1.0), 0.0), scorer(ND)).all(), (metric, qlen)


def test_single_length_corpora_reach_maximum_255_and_256():
    """stream_asm_f64_table serves maxima up to 255: each of its three kinds of maximum has a corpus on either side, and rows that score on both sides of the cutoffs"""
    seen = []
    for case in I.leg_cases("table-edge"):
        for metric in case.metrics:
            seen.append((metric.name, I.maximum(metric, len(case.q), case.len2)))
            full = I.Scorer(metric, case.q, case.corpus)(NS)
            assert len(np.unique(full)) >= 8 and len(case.corpus[1]) % 64 != 0 and len(np.unique(case.corpus[1])) < 64
    by_metric = {}
    for name, mx in seen:
        by_metric.setdefault(name, []).append(mx)
    assert by_metric == {"indel": [255, 256], "ratio(indel)": [255, 256], "levenshtein(1,1,2)": [255, 256], "lcs_seq": [255, 256], "ratio": [255, 256],
                         "levenshtein(5,5,10)": [255, 260]}, by_metric


def test_corpora_are_what_the_legs_say():
    data, offsets, q = I.ragged("alnum", 40)
    lens = np.diff(offsets).astype(np.int64)
    assert len(lens) == I.N_RAGGED and len(lens) % 64 != 0 and lens.min() == 0 and 64 < lens.max() <= 80 and (lens <= 64).mean() > 0.95 and len(q) == 40
    assert set(np.unique(I.ragged("abcd", 5)[0]).tolist()) == set(b"abcd")
    for L, qlen in I.ROW_SHAPES:
        r, q = I.rows(L, qlen)
        assert r.shape == (I.N_ROWS, L) and I.N_ROWS % 64 != 0 and len(np.unique(r)) < 64 and len(q) == qlen
    r, q = I.rows(64, 64)
    assert [int((r[4 * k] != q).sum()) for k in range(8) if k not in (1, 2)] == [k for k in range(8) if k not in (1, 2)]  # exactly k substitutions
    cands, q, symbols = I.chars()
    assert len(q) == 33 and max(int(s) for s in symbols) > 0xFFFF and min(int(s) for s in symbols) > 255 and len(symbols) == 40
    data, offsets, q = I.jaro_multiword()
    lens = np.diff(offsets).astype(np.int64)
    assert len(q) == 100 and len(lens) == 301 and lens.min() >= 60 and lens.max() <= 207 and (lens > 64).mean() > 0.9


def test_no_lcs_family_query_is_longer_than_64():
    """quirk Q8 of the reference's banded multi-word LCS needs a query beyond 64 symbols: it cannot apply, and no mismatch is excused"""
    for leg in I.LEG_NAMES:
        for case in I.leg_cases(leg):
            if any(m.family == "lcs" for m in case.metrics):
                assert len(case.q) <= 64, (leg, case.tag)
            if len(case.q) > 64:
                assert all(m.family == "jaro" for m in case.metrics), (leg, case.tag)


def test_multitile_corpora_give_every_wavefront_two_tiles():
    """the sizing of multitile_cases(): 2 x 4 x CUs + 1 tiles of one length -- per length in the ragged corpus -- and a partial last tile"""
    for cus in (2, 5):
        single, two = list(I.multitile_cases(cus))
        tiles = 2 * 4 * cus + 1
        assert single.min_tiles == two.min_tiles == tiles and len(single.q) == 64
        n = len(single.corpus[1])
        assert -(-n // 64) == tiles and n % 64 != 0 and single.corpus[1].shape[1] == 64
        lens = np.diff(two.corpus[2]).astype(np.int64)
        assert sorted(set(lens.tolist())) == [63, 64] and all(int((lens == L).sum()) // 64 == tiles and int((lens == L).sum()) % 64 != 0 for L in (63, 64))
