"""The inputs of tests/test_gpu_layouts_multi.py (tests/layout_multi_inputs.py) are what that test needs them to be -- checked on the host, without a GPU:
rf.host_layout of the scanned corpus P and of the query corpus QC in one child process per knob setting (the knobs are read once per process), the planted rows,
the length windows a tight cutoff gives on the padded layout, and the CPU oracle's answers to every case the GPU test runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)
import layout_multi_inputs as I  # noqa: E402

KNOBS = {"default": {}, "no_mixed": {"RF_NO_MIXED_TILES": "1"}, "no_rename": {"RF_NO_RENAME": "1"}}
CHILD = ("import sys; sys.path[:0] = [%r, %r]; import numpy as np; import rapidfuzz_rs_amd as rf; import layout_multi_inputs as I\n"
         "out = {}\n"
         "for name, c in (('P', I.scanned()), ('QC', I.query_corpus())):\n"
         "    lay = rf.host_layout(c.data, c.offsets)\n"
         "    for key in ('orig', 'tile_len', 'sigma', 'n_exact', 'n_mixed'):\n"
         "        out[name + '_' + key] = np.asarray(lay[key])\n"
         "np.savez(sys.argv[1], **out)\n") % (ROOT, TESTS)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{knob setting: {P_orig, P_tile_len, P_sigma, P_n_exact, P_n_mixed, QC_...}}"""
    tmp = tmp_path_factory.mktemp("layout_multi")
    out = {}
    for name, env in KNOBS.items():
        path = str(tmp / f"{name}.npz")
        r = subprocess.run([sys.executable, "-c", CHILD, path], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(path) as z:
            out[name] = {k: z[k] for k in z.files}
    return out


def test_the_counts_are_the_designed_ones():
    p, qc = I.scanned(), I.query_corpus()
    lens = np.diff(p.offsets.astype(np.int64))
    counts = np.bincount(lens, minlength=I.MAX_LEN + 1)
    assert len(counts) == I.MAX_LEN + 1 and counts.tolist() == [p.counts[ln] for ln in range(I.MAX_LEN + 1)]
    assert all(c % 64 >= 1 and c // 64 <= 2 for c in counts)
    assert counts[0] == 5 and counts[20] // 64 == 2 and counts[33] == 65 and counts[64] == 2 * 64 + 63 and all(counts[ln] < 64 for ln in range(65, 71))
    assert 6000 <= p.n <= 8000
    assert not np.array_equal(np.sort(lens), lens)  # shuffled
    assert [len(q) for q in I.queries()] == I.QUERY_LENGTHS
    assert qc.counts == I.QC_COUNTS and 140 <= qc.n <= 160
    assert [qc.rows[r] for r in qc.qrow] == I.queries()
    # the symbols: a skewed law, with 0x00 and 0xFF present
    hist = np.bincount(p.data, minlength=256)
    assert hist[0] > 0 and hist[255] > 0 and hist[126] > 0
    top = np.sort(hist)[::-1]
    assert top[0] > 8 * top[40] > 0


def test_the_default_layout_has_a_mixed_section_and_renames(layouts):
    lay = layouts["default"]
    assert int(lay["P_n_mixed"]) > 0 and int(lay["QC_n_mixed"]) > 0
    assert int(lay["QC_n_exact"]) == 2  # one exact tile for each of the lengths 20 and 33
    identity = np.arange(256, dtype=np.uint8)
    assert not np.array_equal(lay["P_sigma"], identity) and not np.array_equal(lay["QC_sigma"], identity)
    assert int((lay["P_sigma"] != identity).sum()) > 60  # far from the identity
    assert not np.array_equal(lay["P_sigma"], lay["QC_sigma"])  # the two sides of a join store different codes


def test_no_rename_stores_the_bytes(layouts):
    lay = layouts["no_rename"]
    identity = np.arange(256, dtype=np.uint8)
    assert np.array_equal(lay["P_sigma"], identity) and np.array_equal(lay["QC_sigma"], identity)
    assert int(lay["P_n_mixed"]) > 0  # (the layout is the default one)


@pytest.mark.parametrize("which", ["P", "QC"])
def test_no_mixed_tiles_pads_every_length(layouts, which):
    lay = layouts["no_mixed"]
    c = I.scanned() if which == "P" else I.query_corpus()
    pad, tile_len = I.pad_map(c.counts)
    assert int(lay[which + "_n_mixed"]) == 0 and int(lay[which + "_n_exact"]) == len(tile_len)
    assert lay[which + "_tile_len"].astype(np.int64).tolist() == tile_len.tolist()  # one ascending run of ceil(count / 64) tiles per length
    orig = lay[which + "_orig"]
    assert len(orig) == len(pad) and np.array_equal(orig == I.NONE32, pad)  # padding exactly at the end of each length's last tile
    assert np.array_equal(np.sort(orig[~pad]), np.arange(c.n, dtype=np.uint32))
    # the tile of length 33 with ONE live lane
    t = int(np.nonzero(tile_len == 33)[0][-1])
    assert int((orig[64 * t: 64 * t + 64] != I.NONE32).sum()) == 1
    # every length ends in a partial tile
    live = (orig.reshape(-1, 64) != I.NONE32).sum(axis=1)
    assert all(live[int(np.nonzero(tile_len == ln)[0][-1])] < 64 for ln in c.counts)


def _tile_of(orig):
    """candidate -> (tile, the tile has padding lanes)"""
    tiles = orig.reshape(-1, 64)
    padded = (tiles == I.NONE32).any(axis=1)
    slot_of = np.empty(int((orig != I.NONE32).sum()), dtype=np.int64)
    real = np.nonzero(orig != I.NONE32)[0]
    slot_of[orig[real]] = real
    return slot_of // 64, padded


def test_every_query_is_planted_in_a_padded_and_in_a_full_tile(layouts):
    p, qs = I.scanned(), I.queries()
    tile, padded = _tile_of(layouts["no_mixed"]["P_orig"])
    seen = set()
    for qi, q in enumerate(qs):
        rows = p.planted[qi]
        assert [k for k, _ in rows] == list(I.PLANT_EDITS)
        kinds = {bool(padded[tile[at]]) for _, at in rows}
        assert kinds == {True, False}, (qi, kinds)
        for k, at in rows:
            assert at not in seen  # no planted row was overwritten
            seen.add(at)
            assert abs(len(p.cands[at]) - len(q)) <= k
            assert I.J.ORA["levenshtein"].distance(q, p.cands[at]) <= k
        assert p.cands[rows[0][1]] == q and p.cands[rows[1][1]] == q
    assert len(seen) == len(qs) * len(I.PLANT_EDITS)
    # the rank rule the inputs were built by is the packer's
    for i in range(0, p.n, 7):
        assert bool(padded[tile[i]]) == I.in_padded_tile(p.rank[i], p.counts[len(p.cands[i])])


def test_the_query_corpus_puts_the_queries_where_the_joins_need_them(layouts):
    qc = I.query_corpus()
    tile, padded = _tile_of(layouts["no_mixed"]["QC_orig"])
    a, b = qc.qrow[3], qc.qrow[4]  # Q's two 20-symbol rows: one in the full tile, one in the partial tile
    assert not padded[tile[a]] and padded[tile[b]]
    live = (layouts["no_mixed"]["QC_orig"].reshape(-1, 64) != I.NONE32).sum(axis=1)
    assert live[tile[qc.qrow[7]]] == 1 and not padded[tile[qc.qrow[6]]]  # Q's second 33-symbol row is the one live lane of its tile
    assert sorted(qc.padded) == [i for i in range(qc.n) if padded[tile[i]]]
    qi = I.join_query_indices()
    assert set(qi) == set(qc.padded) | {qc.qrow[10]} and len(qi) > len(set(qi)) and qi != sorted(qi)
    # in the default layout the same two rows sit in an exact tile and in the mixed section
    lay = layouts["default"]
    tile_d, _ = _tile_of(lay["QC_orig"])
    assert tile_d[a] < int(lay["QC_n_exact"]) <= tile_d[b]


def test_tight_windows_begin_and_end_inside_the_corpus(layouts):
    """Levenshtein distance <= 3 on the padded layout: windows with tile_begin > 0, tile_end < n_tiles and a padded last tile, for a query of either class; in the
    default layout a window that holds a view runs on over later exact tiles or begins before them"""
    p = I.scanned()
    lay = layouts["no_mixed"]
    tile_len = lay["P_tile_len"].astype(np.int64)
    padded = (lay["P_orig"].reshape(-1, 64) == I.NONE32).any(axis=1)
    inside = {True: 0, False: 0}
    for ln in I.QUERY_LENGTHS[:-1]:
        b, e = I.window(tile_len, ln, 3)
        assert b < e and (np.abs(tile_len[b:e] - ln) <= 3).all()
        assert b == 0 or abs(int(tile_len[b - 1]) - ln) > 3
        assert e == len(tile_len) or abs(int(tile_len[e]) - ln) > 3
        if b > 0 and e < len(tile_len) and padded[e - 1]:
            inside[ln <= 32] += 1
    assert inside[True] >= 1 and inside[False] >= 1
    # the default layout: the window of the 20-symbol queries encloses tiles of other lengths
    d_len = layouts["default"]["P_tile_len"].astype(np.int64)
    b, e = I.window(d_len, 20, 3)
    assert b < int(layouts["default"]["P_n_exact"]) < e and (np.abs(d_len[b:e] - 20) > 3).any()
    assert sum(p.counts.values()) == p.n


def _admits(metric, op, cutoff, len1, len2, k):
    """a row at k edits of a query surely passes: Levenshtein and LCS distance <= k, Indel distance <= 2 k"""
    dist = 2 * k if metric == "indel" else k
    maximum = len1 + len2 if metric == "indel" else max(len1, len2)
    return dist <= cutoff if op == I.DIST else maximum - dist >= cutoff


@pytest.mark.parametrize("metric,op,cutoff", I.U32_FILTER + I.U32_PER_QUERY + I.U32_JOIN)
def test_the_oracle_answers_every_u32_case(layouts, metric, op, cutoff):
    p, qs = I.scanned(), I.queries()
    tile, padded = _tile_of(layouts["no_mixed"]["P_orig"])
    total = in_padded = surely = 0
    for qi, q in enumerate(qs):
        idx, _ = I.somes(False, metric, op, cutoff, q)
        have = set(idx.tolist())
        for k, at in p.planted[qi]:
            if _admits("levenshtein" if metric == "osa" else metric, op, cutoff, len(q), len(p.cands[at]), k):
                assert at in have, (qi, k, at)
                surely += 1
        total += len(idx)
        in_padded += int(padded[tile[idx]].sum())
    assert surely >= 6 and 0 < total < len(qs) * p.n and in_padded > 0


@pytest.mark.parametrize("metric,op,cutoff", I.F64_FILTER + I.F64_PER_QUERY + I.F64_JOIN)
def test_the_oracle_answers_every_f64_case(layouts, metric, op, cutoff):
    p, qs = I.scanned(), I.queries()
    tile, padded = _tile_of(layouts["no_mixed"]["P_orig"])
    total = in_padded = 0
    best = I.bits([0.0 if op == I.ND else 1.0])[0]
    for qi, q in enumerate(qs):
        idx, sc = I.somes(True, metric, op, cutoff, q)
        have = dict(zip(idx.tolist(), I.bits(sc)))
        for k, at in p.planted[qi]:
            if k == 0:
                assert have.get(at) == best, (qi, at)  # the copies
        total += len(idx)
        in_padded += int(padded[tile[idx]].sum())
    assert 0 < total < len(qs) * p.n and in_padded > 0


def test_the_joins_of_the_query_corpus_match_in_padded_tiles(layouts):
    """QC x P matches beyond Q's own rows (the filler rows cut from P), P x QC and QC x QC are neither empty nor full"""
    p, qc = I.scanned(), I.query_corpus()
    tile, padded = _tile_of(layouts["no_mixed"]["P_orig"])
    exp = I.oracle_u32("P", "levenshtein", I.DIST, 3).triples(qc.rows)
    own = set(qc.qrow)
    assert sum(1 for t in exp if t[0] not in own) > 50 and sum(1 for t in exp if padded[tile[t[1]]]) > 50
    assert 0 < len(exp) < qc.n * p.n
    # rows of either class match in the LAST tile of their window (three symbols longer, the partial tile of that length) and in its FIRST
    tile_len = layouts["no_mixed"]["P_tile_len"].astype(np.int64)
    last, first = {20: 0, 33: 0}, {20: 0, 33: 0}
    for row, cand, _ in exp:
        ln, cl = len(qc.rows[row]), len(p.cands[cand])
        if ln in last and cl == ln + 3 and padded[tile[cand]]:
            b, e = I.window(tile_len, ln, 3)
            assert tile[cand] == e - 1
            last[ln] += 1
        if ln in first and cl == ln - 3 and tile[cand] == I.window(tile_len, ln, 3)[0]:
            first[ln] += 1
    assert min(last.values()) >= 3 and min(first.values()) >= 3, (last, first)
    back =I.oracle_u32("QC", "levenshtein", I.DIST, 3).triples(p.cands)
    assert 0 < len(back) < qc.n * p.n and sorted((t[1], t[0], t[2]) for t in back) == exp
    self_join = I.oracle_u32("QC", "levenshtein", I.DIST, 3)
    full, upper = self_join.triples(qc.rows), self_join.triples(qc.rows, upper=True)
    assert len(full) > qc.n and 0 < len(upper) and len(full) == qc.n + 2 * len(upper)
