"""tests/call_sequences.py -- the inputs, the catalogue and the schedule of tests/call_sequence_check.py -- held to its own conditions from the CPU side alone: a
schedule that misses an ordered pair, a cutoff nothing passes, two letters with one expected value or a planted row at another distance than its construction says
would leave the GPU test green for the wrong reason."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import call_sequences as S  # noqa: E402
import textbook as tb  # noqa: E402


@pytest.fixture(scope="module")
def cat():
    return S.catalogue()


def test_catalogue_size_and_names(cat):
    names = [lt.name for g in cat.values() for lt in g]
    assert len(set(names)) == len(names)
    for group, ls in cat.items():
        assert 14 <= len(ls) <= 24, (group, len(ls))
        assert all(lt.group == group for lt in ls)
    assert {lt.corpus for lt in cat["W"]} == {"W", "W2"}


def test_schedule_holds_every_ordered_pair_and_is_seeded(cat):
    sched = S.schedule()
    assert sched == S.schedule(S.SEED) and sched != S.schedule(S.SEED + 1)
    for group, ls in cat.items():
        part = [nm for g, nm in sched if g == group]
        names = [lt.name for lt in ls]
        assert len(part) == len(names) ** 2 + 1
        pairs = set(zip(part, part[1:]))
        assert pairs == {(a, b) for a in names for b in names}, (group, len(pairs))
    cross = [nm for g, nm in sched if g == "cross"]
    assert len(cross) == S.CROSS_CALLS
    groups = {nm: lt.group for nm, lt in S.letters().items()}
    assert {groups[nm] for nm in cross} == {"U", "R", "W"} and {S.letters()[nm].corpus for nm in cross} == {"U", "R", "W", "W2"}
    assert sum(groups[a] != groups[b] for a, b in zip(cross, cross[1:])) > S.CROSS_CALLS // 2  # it interleaves


def test_take_runs_on_both_sides_of_the_first_gather_scan(cat):
    part = [nm for g, nm in S.schedule() if g == "R"]
    gather = {lt.name for lt in cat["R"] if "gather" in lt.tags}
    assert gather
    first = min(part.index(nm) for nm in gather)
    assert "r.take" in part[:first] and "r.take" in part[first + 1:]


def test_corpora_meet_their_conditions():
    from rapidfuzz_rs_amd.corpus import host_layout

    u = S.corpus_u()["rows"]
    tiles = (len(u) + 63) // 64
    assert u.shape[1] == 64 and tiles >= 129 and tiles % 2 == 1 and len(u) % 64 != 0 and len(np.unique(u)) < 63
    r = S.corpus_r()
    lens = r["lens"]
    lay = host_layout(r["data"], r["offsets"])
    assert lay["n_exact"] + lay["n_mixed"] >= 129 and lay["n_mixed"] >= 2
    assert np.count_nonzero(lens == 63) // 64 >= 40 and np.count_nonzero(lens == 64) // 64 >= 40
    assert set(range(71)) <= set(lens.tolist()) and np.count_nonzero(lens == 0) >= 1
    w = S.corpus_w()
    for name in ("W", "W2"):
        wl = np.diff(w[name]["offsets"].astype(np.int64))
        assert wl.max() <= 32 and len(set(wl.tolist())) > 8 and len(np.unique(w[name]["data"])) > 254 and w[name]["data"].dtype == np.uint32
    assert len(w["W"]["ids"]) == 254 and len(w["W"]["overflow"]) >= 1
    q = w["queries"]
    assert all(int(s) in w["W"]["ids"] for name in ("wq", "wq3", "wq4") for s in q[name])  # plain queries
    assert sum(int(s) in w["W"]["overflow"] for s in q["wqo"]) == 6  # the overflow query
    stored = [int(s) for s in np.unique(q["wq2"]) if int(s) in w["W"]["ids"] or int(s) in w["W"]["overflow"]]
    assert len(stored) > 254 and len(np.unique(q["wq2"])) > 255 and any(s in w["W"]["overflow"] for s in stored)  # the refused query
    for name in ("U", "R", "W", "W2"):
        assert S.corpus_size(name) <= 10_000


def test_every_cutoff_letter_is_worth_running(cat):
    for ls in cat.values():
        for lt in ls:
            if lt.passing is None:
                continue
            n, m = S.corpus_size(lt.corpus), np.atleast_1d(lt.passing())  # (a multi-query letter: every query's count)
            assert 0.002 * n <= m.min() and m.max() <= 0.5 * n, (lt.name, m, n)
    by = S.letters()
    few = [lt for lt in cat["U"] if "few" in lt.tags]
    assert few and all(lt.passing() <= 64 for lt in few)
    assert S.corpus_u()["carriers"]["many"] * 2 >= S.corpus_size("U") and S.corpus_u()["carriers"]["a"] * 10 <= S.corpus_size("U")
    many = [lt for lt in cat["U"] if "many" in lt.tags]
    assert many and all(lt.passing() > few[0].passing() for lt in many)
    short = by["u.top64<=2.short"]
    assert short.passing() < 64 and len(short.expected[0]) == short.passing()
    assert by["u.filter<=3.many.cap50"].passing() > 50
    assert int(by["r.filter_multi<=3"].expected[0].max()) <= 1024 and int(by["r.filter_multi.nsim>=0.9"].expected[0].max()) <= 1024  # (the capacity the letters pass)
    # the hints, over the rows a hint can bear on: those within max(hint, 31) symbols of the query's length
    lens = S.corpus_r()["lens"]
    reach = np.abs(lens - S.LONG_LEN) <= 31
    assert reach.sum() >= 64 * 40
    right = S.dense("R", "levenshtein", "q200", S.OP_DISTANCE)[reach]
    wrong = S.dense("R", "levenshtein", "q200w", S.OP_DISTANCE)[reach]
    assert np.count_nonzero(right > S.HINT) * 4 <= reach.sum(), np.count_nonzero(right > S.HINT) / reach.sum()
    assert np.count_nonzero(wrong > S.HINT) * 2 >= reach.sum()


def test_the_kept_score_buffer_is_read_after_another_query_wrote_it(cat):
    """The scan-plus-one-pass top-k (a Levenshtein query of 2 to 4 words, no cutoff, k <= 64) keeps its score vector per (corpus, stream): W has two such letters
    with different queries, whose dense vectors differ at the very rows either call returns, and R has one."""
    via = {g: [lt for lt in ls if "via-scores" in lt.tags] for g, ls in cat.items()}
    assert len(via["W"]) >= 2 and len(via["R"]) >= 1
    q = S.all_queries()
    qname = {"r.top16.q200": "q200", "w.top16.wql": "wql", "w.top5.wql2": "wql2"}
    for lt in via["W"] + via["R"]:
        assert 65 <= len(q[qname[lt.name]]) <= 256 and lt.passing is None and 1 <= len(lt.expected[0]) <= 64, lt.name
        if lt.corpus == "W":  # (R's is a list of ties, the exact copies of the query, which the index orders)
            assert len(set(lt.expected[0].tolist())) >= 3, lt.name
    a, b = via["W"]
    da, db = S.dense("W", "levenshtein", qname[a.name], S.OP_DISTANCE), S.dense("W", "levenshtein", qname[b.name], S.OP_DISTANCE)
    for lt, other in ((a, db), (b, da)):  # read from the other query's scores, neither list would come out
        scores, indices = lt.expected
        got = S.topk_of(other, len(scores))
        assert not np.array_equal(got[1], indices) and not np.array_equal(other[indices.astype(np.int64)], scores), lt.name
    w = S.corpus_w()["W"]
    for name in ("wql", "wql2"):
        d = S.dense("W", "levenshtein", name, S.OP_DISTANCE)
        for i, e in w["plants"][name]:
            assert int(d[i]) == S.LONG_W - 24 + e, (name, i, e)


def test_no_two_letters_of_a_group_expect_the_same_value(cat):
    """a result left over from the previous call cannot pass for the current one.  (The letters checked by contract -- a capacity below the count -- deliver
    `capacity` pairs, which no other letter of their group does: their shapes are compared as delivered.)"""
    for group, ls in cat.items():
        seen = []
        for lt in ls:
            if lt.tags & {"novalue", "refused"}:  # (a refusal's value is its status: no result that a buffer could hold)
                continue
            value = lt.expected
            if "cap50" in lt.tags:
                value = (value[0], value[1][:50], value[2][:50])
            for other, v in seen:
                assert not (S.shape_of(v) == S.shape_of(value) and S.same(v, value)), (group, other, lt.name)
            seen.append((lt.name, value))


def test_planted_rows_are_at_the_distance_their_construction_says():
    q = S.all_queries()
    u = S.corpus_u()
    for name, plants in u["plants"].items():
        for i, e in plants:
            assert tb.levenshtein_unit(q[name], u["rows"][i]) == e and tb.indel(q[name], u["rows"][i]) == 2 * e, (name, i, e)
    r = S.corpus_r()
    o = r["offsets"].astype(np.int64)
    for name, plants in r["plants"].items():
        for i, e, ln in plants[::3]:
            row = r["data"][o[i]:o[i + 1]]
            assert len(row) == ln and tb.levenshtein_unit(q[name], row) == e + (64 - ln) and tb.indel(q[name], row) == 2 * e + (64 - ln), (name, i, e, ln)
    for i in u["swaps"]:
        assert (tb.levenshtein_unit(q["b"], u["rows"][i]), tb.osa(q["b"], u["rows"][i])) == (2, 1)
    w = S.corpus_w()["W"]
    ow = w["offsets"].astype(np.int64)
    for name, plants in w["plants"].items():
        for i, e in plants:
            far = S.LONG_W - 24 if name in ("wql", "wql2") else 0  # (the rows of the long queries are 24 of their 100 symbols)
            assert tb.levenshtein_unit(q[name], w["data"][ow[i]:ow[i + 1]]) == far + e, (name, i, e)
    # the dense vectors the letters are derived from say the same
    lev, ind = S.dense("U", "levenshtein", "a", S.OP_DISTANCE), S.dense("U", "indel", "a", S.OP_DISTANCE)
    for i, e in u["plants"]["a"]:
        assert (int(lev[i]), int(ind[i])) == (e, 2 * e)


def test_refusals_and_empty_letters_are_what_the_header_documents(cat):
    by = S.letters()
    assert int(by["w.refused.slot_order"].expected[0][0]) == S.RF_ERR_UNSUPPORTED and int(by["w.refused.symbols"].expected[0][0]) == S.RF_ERR_UNSUPPORTED
    assert int(by["w.refused.jaro_topk_multi"].expected[0][0]) == S.RF_ERR_INVALID_ARG
    assert sum("novalue" in lt.tags for g in cat.values() for lt in g) == 3
