"""The inputs of tests/symbol_edge_check.py put a query symbol on table row 63 (no GPU: the packer's host layout).

The checker's point is that its corpora store exactly D = 62 .. 65 distinct symbols with the D-th one on code D - 1, and that its query families b and d hold
the byte whose code is 63 -- the fill code of the 6-bit payload -- although the corpus does not (D <= 63).  A change to the generators could quietly undo that,
and the GPU legs would stay green for the wrong reason."""
import numpy as np
import pytest

import symbol_edge_check as SE


def _corpora(D, n):
    """(name, flat data, offsets) of the checker's corpora at n candidates"""
    for L in (64, 57, 7):
        rows, q = SE.rows_corpus(D, L, n=n)
        yield f"rows of {L}", rows.reshape(-1), SE.uniform_offsets(rows), q
    for L in (40, 64):
        rows, q = SE.rows_corpus(D, L, n=n, heads=True)
        yield f"head rows of {L}", rows.reshape(-1), SE.uniform_offsets(rows), q
    data, offsets, q = SE.bucketed_corpus(D, n=n)
    yield "bucketed", data, offsets, q


@pytest.mark.parametrize("D", SE.DS)
def test_corpora_store_d_symbols_and_the_queries_hold_the_code_63_byte(D):
    for name, data, offsets, q in _corpora(D, 333):
        present = np.unique(data)
        assert len(present) == D and set(present.tolist()) == set(SE.POOL[:D].tolist()), name
        sigma, b63, b64, b65 = SE.code_bytes(data, offsets)
        assert int(sigma[present].max()) == D - 1, (name, int(sigma[present].max()))
        assert int(sigma[SE.POOL[D - 1]]) == D - 1, name  # the rarest symbol owns the largest code
        assert sorted(sigma[present].tolist()) == list(range(D)), name
        assert (b63 in present) == (D >= 64), (name, b63)
        assert (b64 in present) == (D >= 65) and b65 not in present and 255 not in present, (name, b64, b65)
        assert all(int(sigma[b]) == code for b, code in ((b63, 63), (b64, 64), (b65, 65))), name
        assert q[list(SE.RARE_AT)].tolist() == [SE.POOL[D - 1]] * 2 and set(q.tolist()) <= set(present.tolist()), name
        for ln in (20, 40, 64):
            fam = SE.families(q[:ln], b63, b64, b65)
            assert set(fam["a"].tolist()) <= set(present.tolist()), name
            assert int(np.count_nonzero(fam["b"] == b63)) >= 8 and (fam["b"][-7:] == b63).all(), name
            assert (fam["d"] == b63).all() and len(fam["d"]) == ln, name
            assert {b64, b65, 255} <= set(fam["c"].tolist()), name
            assert all(SE.POOL[D - 1] in fam[f] for f in "abc"), name  # the rarest symbol stays in the query


def test_planted_rows_hold_the_rarest_symbol_where_the_query_does():
    for D in SE.DS:
        rare = SE.POOL[D - 1]
        rows, q = SE.rows_corpus(D, 64, n=SE.N)
        planted = rows[SE.PLANT_EVERY // 2::SE.PLANT_EVERY]
        keep = (planted[:, list(SE.RARE_AT)] == rare).all(axis=1)
        assert 3 <= keep.sum() < len(planted)  # some keep it, the others hold a common symbol there
        rows, q = SE.rows_corpus(D, 64, n=SE.N, heads=True)
        planted = rows[SE.PLANT_EVERY // 2::SE.PLANT_EVERY]
        assert len(planted) >= 8  # every kind of head edit once
        assert ((planted[:, :8] != q[:8]).sum(axis=1) > 0).sum() >= 6 and (planted[:, :8] == rare).any(axis=1).sum() >= 8


def test_road_tables_follow_the_issue():
    # (largest stored code, length) -> 6-bit payload; the partial-chunk row is the one that differs
    assert [SE.expect_data6(D - 1, 64) for D in SE.DS] == [1, 1, 1, 0]
    assert [SE.expect_data6(D - 1, 57) for D in SE.DS] == [1, 1, 0, 0]
    assert [SE.expect_data6(D - 1, 7) for D in SE.DS] == [1, 1, 0, 0]
    assert [SE.expect_data6_bucketed(D - 1, False) for D in SE.DS] == [1, 1, 1, 0] and not any(SE.expect_data6_bucketed(D - 1, True) for D in SE.DS)
    assert [SE.expect_heads6(D - 1) for D in SE.DS] == [1, 1, 1, 0]
    assert [(SE.expect_data6(t, 57), SE.expect_data6(t, 64), SE.expect_heads6(t)) for t in SE.NORENAME_TOPS] == [(1, 1, 1), (0, 1, 1), (0, 0, 0)]


def test_norename_corpora_reach_the_bounds_by_value():
    for top in SE.NORENAME_TOPS:
        for L in (57, 64):
            rows, q = SE.norename_corpus(top, L, n=333)
            assert int(rows.max()) == top and len(np.unique(rows)) == 10 and q[list(SE.RARE_AT)].tolist() == [top, top]
            assert all(63 in SE.families(q[:ln], 63, 64, 65)[f] for ln in (20, 40) for f in "bd")


def test_the_checker_knows_the_status_that_ends_a_leg():
    from rapidfuzz_rs_amd import _native as N

    assert SE.RF_ERR_HIP == N.RF_ERR_HIP
