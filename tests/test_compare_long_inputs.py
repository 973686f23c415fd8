"""The cases of tests/compare_long_inputs.py reach what tests/test_gpu_compare_long.py and tests/compare_long_check.py need them for (no GPU: the reference of
tests/compare_reference.py alone).

The GPU legs compare the device with the reference by bits.  A change to a generator could quietly drop the chunk-row counts that make hamming's unrolled loop
run twice, the shifts of postfix, or the one live lane of an early-out tile, and the GPU legs would stay green for the wrong reason: the conditions are
asserted here.  Measured on one CPU core: 8 s for this file, 4.6 s of it in the test that first needs the raw values of every case."""
import numpy as np
import pytest

import compare_long_inputs as L
import compare_reference as R


def _lens(name):
    return np.array([len(c) for c in L.case(name).cands], dtype=np.int64)


def test_every_corpus_has_full_tiles_and_a_partial_one():
    for name in L.all_cases():
        n = len(L.case(name).cands)
        assert n >= 65 and 1 <= n % 64 <= 63, (name, n)
    for q, names in L.length_cases().items():
        for name in names:
            assert len(L.case(name).cands) == L.n_candidates(int(_lens(name).max())), name  # 64 x 5 + 7 below 1000 symbols, 64 + 3 from there on
            assert list(L.case(name).queries) == [q]
        lens = _lens(f"ragged-{q}")
        assert (lens == q).sum() >= 64 and (lens < q).any() and (lens > q).any()  # straddles: a whole tile of the query's length, and both sides of it


def test_ragged_cases_pack_to_exact_tiles_and_a_mixed_section():
    from rapidfuzz_rs_amd.corpus import host_layout, ragged

    for name in [f"ragged-{q}" for q in L.QUERY_LENS] + ["shift", "longcand", "road", "order", "all256-40", "all256-300"]:
        lay = host_layout(*ragged(L.case(name).cands))
        assert lay["n_exact"] >= 1 and lay["n_mixed"] >= 1 and not lay["identity"], (name, lay["n_exact"], lay["n_mixed"])
    lay = host_layout(*ragged(L.case("shift").cands))
    assert lay["n_exact"] == 16 * 2 + 6 + 2


def test_hamming_chunk_row_counts():
    seen = {}
    for name in [n for names in L.length_cases().values() for n in names] + L.EXTRA_CASES:
        (q,) = L.case(name).queries
        for len2 in set(_lens(name).tolist()):
            if len2 == q:  # (strict and padded both count these rows; the padded run also covers min(len1, len2) of the neighbours)
                seen.setdefault(L.nch(q), set()).add(q)
    assert L.HAMMING_NCH <= set(seen), sorted(seen)
    passes = {L.hamming_passes(m)[0] for ms in seen.values() for m in ms}
    assert {1, 2, 3, 15} <= passes and max(passes) >= 63
    tails_after_two = {L.hamming_passes(m)[1] for ms in seen.values() for m in ms if L.hamming_passes(m)[0] >= 2}
    assert tails_after_two == {1, 2, 3, 4}
    # the kernel's own loop, restated: c + 4 < nch
    for m in (80, 81, 160, 4097):
        c = 0
        while c + 4 < L.nch(m):
            c += 4
        assert (c // 4, L.nch(m) - c) == L.hamming_passes(m)
    # m on a multiple of 16 and on either side of it: equal lengths above it, and below it the padded run over the neighbouring single-length corpus
    ms = {m for v in seen.values() for m in v}
    padded = {min(q, int(len2)) for q, names in L.length_cases().items() for name in names for len2 in set(_lens(name).tolist())}
    for mult in (80, 128, 4096):
        assert mult in ms and mult + 1 in ms and mult - 1 in padded


def test_postfix_shifts():
    lens = _lens("shift")
    assert set(lens.tolist()) == set(L.SHIFT_LENGTHS) | {300} and lens.min() >= 200
    for q in (230, 190):
        sign = 1 if q == 230 else -1
        lengths = [v for v in L.SHIFT_LENGTHS if (q - v) * sign > 0]
        assert {(q - v) % 16 for v in lengths} == set(range(16)), q
        for v in lengths:
            assert (lens == v).sum() >= 64 + 1
    # a short query under long candidates: only the last rows of the tile are read (c_lo = (len2 - len1) / 16 >= 17), at a negative shift of hundreds
    assert 23 in L.case("shift").queries and (lens == 300).sum() >= 64 and (300 - 23) // 16 >= 17
    r = L.raw("shift", "postfix", 23)
    assert (r[lens == 300] > 0).sum() >= 5
    # the mirror: a long query, the candidates at most 23 symbols
    (q,) = L.case("mirror").queries
    assert q >= 300 and _lens("mirror").max() <= 23


def _tile(name, label, metric, t):
    return L.raw(name, metric, label)[64 * t: 64 * t + 64]


@pytest.mark.parametrize("name,label,through", [("earlyout", 4100, 4000), ("mtsingle", 1000, 1000), ("shift", 300, 300)])
def test_early_out_tiles(name, label, through):
    lens = _lens(name)
    assert (lens[: 64 * 4] == label).all()
    # exactly one lane matches through `through` symbols or more, the other 63 leave within the first row (prefix) / the last row (postfix)
    last_row = label - 16 * ((label - 1) // 16)
    for metric, t, bound in (("prefix", 0, 16), ("postfix", 1, last_row)):
        r = _tile(name, label, metric, t)
        assert (r >= through).sum() == 1 and (r < bound).sum() == 63, (metric, r)
    # the lanes leave at ten or more distinct depths
    assert len(set((_tile(name, label, "prefix", 2) // 16).tolist())) >= 10
    assert len(set(((label - 1) // 16 - (label - 1 - _tile(name, label, "postfix", 3)) // 16).tolist())) >= 10
    if name != "earlyout":  # the one-live-lane tiles t = 0, 1 come directly before a tile where every lane matches fully: t + 4 on a one-workgroup launch
        assert (lens[64 * 4: 64 * 6] == label).all()
        for metric in ("prefix", "postfix"):
            assert (_tile(name, label, metric, 4) == label).all() and (_tile(name, label, metric, 5) == label).all()
    if name == "earlyout":
        assert label - last_row >= 4000


def test_spread_of_values():
    for name in L.all_cases():
        c = L.case(name)
        lens = _lens(name)
        some = np.zeros(len(c.cands), dtype=bool)
        for label, q in c.queries.items():
            if not len(q):
                continue
            for metric in ("prefix", "postfix"):
                r = L.raw(name, metric, label)
                some |= r > 0
                assert len(set(r.tolist())) >= 3, (name, label, metric)
            equal = lens == len(q)
            if equal.sum() >= 10:
                assert len(set(L.raw(name, "hamming", label)[equal].tolist())) >= 3, (name, label)
        assert 6 * some.sum() >= len(c.cands), (name, int(some.sum()))
        if len(c.queries) == 1:  # ... and per metric where the corpus was built around one query
            (label,) = c.queries
            for metric in ("prefix", "postfix"):
                assert 6 * (L.raw(name, metric, label) > 0).sum() >= len(c.cands), (name, metric)


def test_the_vectorised_reference_equals_the_plain_loop_on_a_sample():
    for name in L.all_cases():
        c = L.case(name)
        n = len(c.cands)
        for label, q in c.queries.items():
            ql = q.tolist()
            for metric in R.METRICS:
                r = L.raw(name, metric, label)
                for i in (0, 1, 64, n // 3, n // 2 + 1, n - 2, n - 1):
                    assert int(r[i]) == R.pair(metric, ql, c.cands[i].tolist()), (name, label, metric, i)


@pytest.mark.parametrize("length", [40, 300])
def test_the_256_symbol_cases(length):
    c = L.case(f"all256-{length}")
    (q,) = c.queries.values()
    assert set(np.concatenate(c.cands).tolist()) == set(range(256))
    for v in (0x00, 0xFF):
        assert v in q.tolist()
        assert sum(1 for x in c.cands if len(x) and x[0] == v) >= 2 and sum(1 for x in c.cands if len(x) and x[-1] == v) >= 2
    assert q[0] == 0x00 and q[-1] == 0xFF  # ... so the edge bytes of the copies decide their affixes
    r = L.raw(c.name, "prefix", length)
    assert (r == length).any() and (r[-8:] == 0).any()


def test_the_char_cases():
    for name in ("char40-300", "char40-5000", "charover-300", "charover-5000"):
        c = L.case(name)
        assert c.wide and all(x.dtype == np.uint32 for x in c.cands)
        held = set(np.concatenate(c.cands).tolist())
        assert len(set(c.queries["absent"].tolist()) - held) == 1 and set(c.queries["main"].tolist()) <= held
        if name.startswith("charover"):
            assert len(held) == 290
            values, counts = np.unique(np.concatenate(c.cands), return_counts=True)
            order = np.argsort(-counts, kind="stable")
            lumped = set(values[order[254:]].tolist())  # whatever the ties: the 36 rarest symbols occur less often than the 254th
            assert counts[order[253]] > counts[order[254]]
            q = c.queries["main"]
            assert {int(q[3]), int(q[len(q) - 4]), int(c.cands[-2][3]), int(c.cands[-1][len(q) - 4])} <= lumped
            # two overflow-class symbols decide: the query itself, the query with q[3] replaced, the query with q[len - 4] replaced
            assert L.raw(name, "prefix", "main")[-3:].tolist() == [len(q), 3, len(q) - 4]
            assert L.raw(name, "postfix", "main")[-3:].tolist() == [len(q), len(q) - 4, 3]
            assert L.raw(name, "hamming", "main")[-3:].tolist() == [0, 1, 1]
        else:
            assert len(held) == 40
