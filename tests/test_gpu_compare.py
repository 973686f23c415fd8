"""hamming / prefix / postfix BatchComparators on the device (rf_compare.hip), BIT-exact against tests/compare_reference.py (which tests/test_compare_reference.py
holds to the reference's known answers and to the oracle): candidate lengths around every chunk boundary x query lengths shorter, equal and longer, single-length
and ragged corpora (exact tiles and mixed blocks), planted mismatches at the chunk edges, the symbol that renames to id 0, the wavefront early-out, all four
ops with cutoffs at an attained value and either side of it, hamming with and without RF_FLAG_HAMMING_PAD -- the two encodings of Err(DifferentLengthArgs) on the
per-candidate roads, never on the selecting ones -- u32 corpora, and every result road.  Several tiles per wavefront: tests/compare_check.py in a child process.

"By bits": the f64 results are compared as u64, so the None NaN and the Err NaN are different values here."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

import compare_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOD = {"hamming": rf.distance.hamming, "prefix": rf.distance.prefix, "postfix": rf.distance.postfix}
OPS = (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY)
CAND_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65]
QUERY_LENS = [0, 1, 15, 16, 17, 23, 40, 64, 65, 66]
KNOWN = json.load(open(os.path.join(ROOT, "tests", "golden", "compare_known_answers.json"), encoding="utf-8"))
PAD = rf.Args().pad()


def _variants(metric):
    """(label, Args or None, pad) -- hamming runs with and without the pad flag"""
    return [("", None, False)] if metric != "hamming" else [("strict", None, False), ("pad", PAD, True)]


def _eq(got, exp, what):
    bad = R.same_bits(got, exp)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:5]}: got {got[bad[:5]]}, expected {exp[bad[:5]]}"


def _near(rng, q, length, sym, how):
    """a candidate of `length` symbols related to the query: it shares a prefix, a suffix, or the positions of the query with a few symbols replaced"""
    q = list(q)
    fill = [int(v) for v in rng.integers(sym, size=length)]
    if not q or not length:
        return fill
    if how == 0:  # common prefix of a random length, then noise
        p = int(rng.integers(0, min(len(q), length) + 1))
        return (q[:p] + fill[p:])[:length]
    if how == 1:  # common suffix
        p = int(rng.integers(0, min(len(q), length) + 1))
        return (fill[: length - p] + q[len(q) - p:])[:length] if p else fill
    if how == 2:  # the query's positions (left-aligned), a few replaced
        c = (q + fill)[:length]
        for pos in rng.integers(0, length, size=int(rng.integers(0, 4))):
            c[int(pos)] = int(rng.integers(sym))
        return c
    c = (fill + q)[-length:]  # right-aligned, a few replaced
    for pos in rng.integers(0, length, size=int(rng.integers(0, 3))):
        c[int(pos)] = int(rng.integers(sym))
    return c


def _make(rng, q, lengths_of, sym=20):
    return [_near(rng, q, L, sym, i % 6) if i % 6 < 4 else [int(v) for v in rng.integers(sym, size=L)] for i, L in enumerate(lengths_of)]


def _bytes_corpus(cands, base=97):
    corpus = rf.Corpus.from_list([bytes(base + v for v in c) for c in cands])
    rows, lens = R.pad_rows([[base + v for v in c] for c in cands])
    return corpus, rows, lens


def _cutoffs(op, uncut):
    """an attained value and one on either side of it; for the normalized ops 0.0, 0.5, 1.0 and a value equal to an attained score"""
    some = uncut[R.keep(uncut)]
    if op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        if not some.size:
            return [0, 1]
        v = int(np.sort(some)[some.size // 2])
        return sorted({max(v - 1, 0), v, v + 1})
    cs = [0.0, 0.5, 1.0]
    if some.size:
        cs.append(float(np.sort(some)[some.size // 2]))
    return cs


def _parity(metric, q, corpus, rows, lens, what, base=97):
    qb = bytes(base + v for v in q)
    qv = [base + v for v in q]
    raw = R.raw_many(metric, qv, rows, lens)
    bc = MOD[metric].BatchComparator(qb)
    for label, args, pad in _variants(metric):
        for op in OPS:
            uncut = R.ops(metric, op, qv, rows, lens, None, pad, raw)
            _eq(bc.many(op, corpus, args), uncut, f"{what} {metric} {label} op {op}")
            for c in _cutoffs(op, uncut):
                _eq(bc.many(op, corpus, args, score_cutoff=c), R.ops(metric, op, qv, rows, lens, c, pad, raw), f"{what} {metric} {label} op {op} cutoff {c}")
    return raw


# ------------------------------------------------------------------------------------------------ known answers
def test_known_answers_through_the_device():
    for e in KNOWN:
        mod = MOD[e["metric"]]
        a, b = e["s1"], e["s2"]
        if not isinstance(a, str):
            a, b = bytes(a), bytes(b)
        args = rf.Args().pad(True) if e["pad"] else None
        fn = getattr(mod.BatchComparator(a), e["op"])
        if e["expect"] == "DifferentLengthArgs":
            with pytest.raises(N.RfError, match="Differing length arguments provided"):
                fn(b, args, score_cutoff=e["cutoff"])
        else:
            assert fn(b, args, score_cutoff=e["cutoff"]) == e["expect"], e
    assert rf.distance.prefix.similarity("prefix", "preference") == 4 and rf.distance.postfix.similarity("postfix", "prefix") == 3
    assert rf.distance.hamming.distance("hamming", "h香mmüng") == 2


# ------------------------------------------------------------------------------------------------ single-length corpora: 64 x 5 + 7 candidates of every length
@pytest.mark.parametrize("len2", CAND_LENS)
def test_single_length_corpora(len2):
    n = 64 * 5 + 7
    for metric in R.METRICS:
        for qlen in QUERY_LENS:
            rng = np.random.default_rng(1000 * len2 + qlen)
            q = [int(v) for v in rng.integers(20, size=qlen)]
            cands = _make(rng, q, [len2] * n)
            corpus, rows, lens = _bytes_corpus(cands)
            raw = _parity(metric, q, corpus, rows, lens, f"single length {len2} query {qlen}")
            if metric != "hamming" and min(len2, qlen) >= 15:
                assert (raw > 0).sum() >= n // 6 and len(set(raw.tolist())) >= 3  # a condition on the inputs: the affixes differ


# ------------------------------------------------------------------------------------------------ ragged: exact tiles, mixed blocks, every (len1 - len2) mod 16
def _ragged_lengths():
    return [L for L in (16, 23, 40) for _ in range(70)] + [L for L in range(0, 67) for _ in range(3)] + [L for L in range(1, 41) for _ in range(2)]


@pytest.mark.parametrize("qlen", QUERY_LENS)
def test_ragged_corpus_with_exact_tiles_and_mixed_blocks(qlen):
    rng = np.random.default_rng(77 + qlen)
    q = [int(v) for v in rng.integers(20, size=qlen)]
    lengths = _ragged_lengths()
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    cands = _make(rng, q, lengths)
    corpus, rows, lens = _bytes_corpus(cands)
    from rapidfuzz_rs_amd.corpus import host_layout, ragged

    lay = host_layout(*ragged([bytes(97 + v for v in c) for c in cands]))  # the layout this test is about: whole tiles of one length AND blocks that mix lengths
    assert lay["n_exact"] >= 3 and lay["n_mixed"] >= 1 and not lay["identity"]
    if qlen == 23:
        assert {(23 - L) % 16 for L in range(1, 41)} == set(range(16))
    for metric in R.METRICS:
        _parity(metric, q, corpus, rows, lens, f"ragged query {qlen}")
    # hamming without pad: the Err encodings sit exactly on the lengths that differ, None only above a cutoff
    bc = rf.distance.hamming.BatchComparator(bytes(97 + v for v in q))
    differ = np.asarray(lens) != qlen
    got = bc.many(N.OP_DISTANCE, corpus, score_cutoff=1)
    assert ((got == N.DIFFERENT_LENGTH_U32) == differ).all()
    assert ((got == N.NONE_U32) <= ~differ).all()
    gotf = bc.many(N.OP_NORMALIZED_SIMILARITY, corpus, score_cutoff=0.9).view(np.uint64)
    assert ((gotf == N.DIFFERENT_LENGTH_F64_BITS) == differ).all() and ((gotf == N.NONE_F64_BITS) <= ~differ).all()
    assert not (bc.many(N.OP_DISTANCE, corpus, PAD) == N.DIFFERENT_LENGTH_U32).any()


# ------------------------------------------------------------------------------------------------ planted cases
@pytest.mark.parametrize("qlen,len2", [(40, 40), (17, 33), (33, 17), (64, 65), (66, 64), (16, 16)])
def test_a_single_mismatch_at_the_chunk_edges(qlen, len2):
    rng = np.random.default_rng(qlen * 100 + len2)
    q = [int(v) for v in rng.integers(20, size=qlen)]
    m = min(qlen, len2)
    cands, expect = [], {"prefix": [], "postfix": []}
    for pos in sorted({0, 15, 16, m - 1} & set(range(m))):
        # left-aligned copy of the query with position `pos` replaced by a symbol outside the alphabet; the tail beyond the query is foreign too
        c = (q + [21] * len2)[:len2]
        c[pos] = 22
        cands.append(c)
        expect["prefix"].append(pos)
        # right-aligned copy with the position `pos` FROM THE END replaced
        c = ([21] * len2 + q)[-len2:]
        c[len2 - 1 - pos] = 22
        cands.append(c)
        expect["postfix"].append(pos)
    cands += [[21] * len2] * 70  # (fill the tile; a second tile)
    corpus, rows, lens = _bytes_corpus(cands)
    qv = [97 + v for v in q]
    assert R.raw_many("prefix", qv, rows, lens)[0 : 2 * len(expect["prefix"]) : 2].tolist() == expect["prefix"]
    assert R.raw_many("postfix", qv, rows, lens)[1 : 2 * len(expect["postfix"]) : 2].tolist() == expect["postfix"]
    for metric in R.METRICS:
        _parity(metric, q, corpus, rows, lens, f"edge mismatches {qlen} x {len2}")


@pytest.mark.parametrize("len2", [1, 15, 16, 17, 40])
def test_the_symbol_that_renames_to_id_zero(len2):
    """a corpus of ONE repeated symbol -- the most frequent one, stored as 0, which is also the value of the padding behind every candidate -- against a longer
    query of that symbol: the scans must stop at len2 by the LENGTH"""
    n = 64 + 9
    cands = [[0] * len2] * n
    corpus, rows, lens = _bytes_corpus(cands)
    for qlen in (len2 + 1, len2 + 16, 66):
        q = [0] * qlen
        qb = bytes(97 + v for v in q)
        assert rf.distance.prefix.BatchComparator(qb).similarity_many(corpus).tolist() == [len2] * n
        assert rf.distance.postfix.BatchComparator(qb).similarity_many(corpus).tolist() == [len2] * n
        assert rf.distance.hamming.BatchComparator(qb).distance_many(corpus, PAD).tolist() == [qlen - len2] * n
        for metric in R.METRICS:
            _parity(metric, q, corpus, rows, lens, f"one symbol, {len2} against {qlen}")
    # ... and the mirror image: candidates longer than the query
    q = [0] * max(len2 - 1, 0)
    for metric in R.METRICS:
        _parity(metric, q, corpus, rows, lens, f"one symbol, {len2} against {len(q)}")


@pytest.mark.parametrize("lane", [0, 31, 63])
def test_the_wavefront_early_out_does_not_cut_the_last_live_lane(lane):
    """63 lanes of a tile mismatch at their first (prefix) / last (postfix) symbol, one lane matches through 40 symbols"""
    rng = np.random.default_rng(lane)
    q = [int(v) for v in rng.integers(20, size=40)]
    for metric, bad_pos in (("prefix", 0), ("postfix", 39)):
        cands = []
        for i in range(64):
            c = list(q)
            if i != lane:
                c[bad_pos] = 21
            cands.append(c)
        corpus, rows, lens = _bytes_corpus(cands)
        got = MOD[metric].BatchComparator(bytes(97 + v for v in q)).similarity_many(corpus)
        assert got.tolist() == [40 if i == lane else 0 for i in range(64)]
        _parity(metric, q, corpus, rows, lens, f"early-out lane {lane}")
        # the same with the one matching lane ending in a mismatch inside the third chunk
        cands[lane] = list(q)
        cands[lane][33 if metric == "prefix" else 6] = 21
        corpus, rows, lens = _bytes_corpus(cands)
        got = MOD[metric].BatchComparator(bytes(97 + v for v in q)).similarity_many(corpus)
        assert got.tolist() == [33 if i == lane else 0 for i in range(64)]


# ------------------------------------------------------------------------------------------------ the roads
def _road_case(seed, qlen=23):
    rng = np.random.default_rng(seed)
    q = [int(v) for v in rng.integers(20, size=qlen)]
    lengths = _ragged_lengths()
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    cands = _make(rng, q, lengths)
    return q, cands


def _road_cutoffs(metric, op, exp_uncut):
    some = exp_uncut[R.keep(exp_uncut)]
    if op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        return [None, int(np.sort(some)[some.size // 3])]
    return [None, 0.5, float(np.sort(some)[some.size // 2])]


def _best_first(exp, some, op):
    desc = op in (N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY)
    return sorted(some.tolist(), key=lambda i: ((-float(exp[i]) if desc else float(exp[i])), i))


@pytest.mark.parametrize("metric", R.METRICS)
def test_filter_in_all_three_orders_never_returns_an_err_candidate(metric):
    q, cands = _road_case(21)
    corpus, rows, lens = _bytes_corpus(cands)
    qv = [97 + v for v in q]
    bc = MOD[metric].BatchComparator(bytes(qv))
    for label, args, pad in _variants(metric):
        for op in OPS:
            for cutoff in _road_cutoffs(metric, op, R.ops(metric, op, qv, rows, lens, None, pad)):
                exp = R.ops(metric, op, qv, rows, lens, cutoff, pad)
                some = R.keep(exp)
                if metric == "hamming" and not pad:
                    assert some.size < len(cands) // 4 and (np.asarray(lens)[some] == len(q)).all()  # the inputs: most candidates are Err
                idx, sc = bc.filter_many(op, corpus, args, score_cutoff=cutoff, order=N.FILTER_BY_INDEX)
                assert idx.tolist() == some.tolist(), (metric, label, op, cutoff)
                _eq(sc, exp[some], f"filter by index {metric} {label} op {op} cutoff {cutoff}")
                assert bc.last_filter_count == some.size
                order = _best_first(exp, some, op)
                idx, sc = bc.filter_many(op, corpus, args, score_cutoff=cutoff, order=N.FILTER_BY_SCORE)
                assert idx.tolist() == order, (metric, label, op, cutoff)
                _eq(sc, exp[order], f"filter by score {metric} {label} op {op} cutoff {cutoff}")
                idx, sc = bc.filter_many(op, corpus, args, score_cutoff=cutoff, order=N.FILTER_ANY)
                assert sorted(idx.tolist()) == some.tolist()
                _eq(sc, exp[idx.astype(np.int64)], f"filter any {metric} {label} op {op} cutoff {cutoff}")


@pytest.mark.parametrize("k", [1, 5, 100])
@pytest.mark.parametrize("metric", R.METRICS)
def test_topk_with_ties_by_index_never_returns_an_err_candidate(metric, k):
    q, cands = _road_case(22)
    corpus, rows, lens = _bytes_corpus(cands)
    qv = [97 + v for v in q]
    bc = MOD[metric].BatchComparator(bytes(qv))
    for label, args, pad in _variants(metric):
        for op in OPS:
            for cutoff in _road_cutoffs(metric, op, R.ops(metric, op, qv, rows, lens, None, pad)):
                exp = R.ops(metric, op, qv, rows, lens, cutoff, pad)
                order = _best_first(exp, R.keep(exp), op)[:k]
                if k == 5 and cutoff is None:
                    assert len(set(exp[_best_first(exp, R.keep(exp), op)[:40]].tolist())) < 40  # the inputs: there are ties to break
                scores, idx = bc.topk(corpus, k, op=op, args=args, score_cutoff=cutoff)
                assert idx.tolist() == order, (metric, label, op, cutoff, k)
                _eq(scores, exp[order], f"topk {metric} {label} op {op} cutoff {cutoff} k {k}")
    # the entries form, which follows the same selection
    import torch

    for label, args, pad in _variants(metric):
        exp = R.ops(metric, N.OP_DISTANCE, qv, rows, lens, None, pad)
        order = _best_first(exp, R.keep(exp), N.OP_DISTANCE)[:k]
        entries = torch.empty((k, 2), dtype=torch.int64, device="cuda")
        bc.topk_entries_device(corpus, k, entries, op=N.OP_DISTANCE, args=args)
        torch.cuda.synchronize()
        got = entries.cpu().numpy()
        assert got[: len(order), 1].tolist() == order and (got[len(order):] == -1).all()


@pytest.mark.parametrize("metric", R.METRICS)
def test_the_multi_calls_with_mixed_query_lengths(metric):
    q, cands = _road_case(23)
    corpus, rows, lens = _bytes_corpus(cands)
    rng = np.random.default_rng(24)
    qs = [q, q[:16], [int(v) for v in rng.integers(20, size=40)], q + q, []]
    cls = MOD[metric].BatchComparator
    bcs = [cls(bytes(97 + v for v in x)) for x in qs]
    for label, args, pad in _variants(metric):
        for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 3), (N.OP_NORMALIZED_DISTANCE, 0.8), (N.OP_NORMALIZED_SIMILARITY, None)):
            exps = [R.ops(metric, op, [97 + v for v in x], rows, lens, cutoff, pad) for x in qs]
            got = cls.many_multi(bcs, op, corpus, args, score_cutoff=cutoff)
            for j in range(len(qs)):
                _eq(got[j], exps[j], f"many_multi {metric} {label} row {j} op {op} cutoff {cutoff}")  # (the Err encodings included)
            tk = cls.topk_multi(bcs, corpus, 5, op=op, args=args, score_cutoff=cutoff)
            fm = cls.filter_multi(bcs, op, corpus, args, score_cutoff=cutoff, order=N.FILTER_BY_INDEX)
            for j in range(len(qs)):
                some = R.keep(exps[j])
                order = _best_first(exps[j], some, op)[:5]
                assert tk[j][1].tolist() == order, (metric, label, j, op, cutoff)
                _eq(tk[j][0], exps[j][order], f"topk_multi {metric} {label} row {j} op {op}")
                assert fm[j][0].tolist() == some.tolist(), (metric, label, j, op, cutoff)
                _eq(fm[j][1], exps[j][some], f"filter_multi {metric} {label} row {j} op {op}")


@pytest.mark.parametrize("metric", R.METRICS)
def test_slot_order_stream_many_and_an_empty_corpus(metric, tmp_path):
    q, cands = _road_case(25)
    corpus, rows, lens = _bytes_corpus(cands)
    qv = [97 + v for v in q]
    bc = MOD[metric].BatchComparator(bytes(qv))
    slots = corpus.slot_index()
    real = np.nonzero(slots != 0xFFFFFFFF)[0]
    assert real.size == len(cands) and corpus.slot_count > len(cands)
    path = str(tmp_path / "compare.rfc")
    corpus.save(path)
    empty = rf.Corpus.from_list([])
    for label, args, pad in _variants(metric):
        for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 2), (N.OP_NORMALIZED_DISTANCE, 0.7)):
            exp = R.ops(metric, op, qv, rows, lens, cutoff, pad)
            got = bc.many(op, corpus, (args or rf.Args()).slot_order(), score_cutoff=cutoff)
            assert got.size == corpus.slot_count
            _eq(got[real], exp[slots[real].astype(np.int64)], f"slot order {metric} {label} op {op}")
            _eq(bc.stream_many(op, path, args=args, score_cutoff=cutoff, segment_bytes=8192), exp, f"stream_many {metric} {label} op {op}")
            assert bc.many(op, empty, args, score_cutoff=cutoff).size == 0
            idx, sc = bc.filter_many(op, empty, args, score_cutoff=cutoff)
            assert idx.size == 0 and sc.size == 0
            scores, idx = bc.topk(empty, 5, op=op, args=args, score_cutoff=cutoff)
            assert scores.size == 0 and idx.size == 0


def test_rf_one_values_and_the_different_length_error():
    L = N.lib()
    a = N.RfArgs()
    L.rf_args_default(C.byref(a))
    v32, vf, some = C.c_uint32(), C.c_double(), C.c_int()

    def one(metric, q, s, op, flags=0, cutoff=None):
        bc = MOD[metric].BatchComparator(q)
        a.flags = flags
        a.cutoff_usize = N.NO_CUTOFF if cutoff is None else cutoff
        buf = (C.c_uint8 * max(1, len(s))).from_buffer_copy(s or b"\0")
        st = L.rf_one_u32(bc._h, buf, len(s), op, C.byref(a), 0, C.byref(v32), C.byref(some))
        return st, v32.value, some.value

    assert one("hamming", b"hamming", b"hammers", N.OP_DISTANCE) == (N.RF_OK, 3, 1)
    assert one("hamming", b"hamming", b"hammers", N.OP_DISTANCE, cutoff=2) == (N.RF_OK, N.NONE_U32, 0)
    assert one("hamming", b"ham", b"hamming", N.OP_DISTANCE, N.FLAG_HAMMING_PAD) == (N.RF_OK, 4, 1)
    assert one("hamming", b"ham", b"hamming", N.OP_DISTANCE)[0] == N.RF_ERR_INVALID_ARG
    assert L.rf_last_error().decode() == "Differing length arguments provided"
    assert one("prefix", b"prefix", b"preference", N.OP_SIMILARITY) == (N.RF_OK, 4, 1)
    assert one("postfix", b"postfix", b"prefix", N.OP_SIMILARITY) == (N.RF_OK, 3, 1)
    assert one("postfix", b"postfix", b"prefix", N.OP_DISTANCE) == (N.RF_OK, 4, 1)
    # the Python single-candidate methods raise for the Err, the normalized ops too
    with pytest.raises(N.RfError, match="Differing length"):
        rf.distance.hamming.normalized_similarity(b"ham", b"hamming")
    assert rf.distance.hamming.normalized_distance(b"ham", b"hamming", PAD) == 4 / 7


# ------------------------------------------------------------------------------------------------ u32 (`char`) corpora
def _chars(c):
    return "".join(map(chr, c))


@pytest.mark.parametrize("metric", R.METRICS)
def test_char_corpora(metric):
    rng = np.random.default_rng(31)
    alphabet = [ord(c) for c in "абвгдежзийклмнопрстуфхцчшщъыьэюя香üAbc1"]
    q = [alphabet[i] for i in rng.integers(len(alphabet), size=23)]
    lengths = [23] * 70 + [int(v) for v in rng.integers(0, 50, size=200)]
    idx_q = [alphabet.index(s) for s in q]
    cands = [[alphabet[v] for v in c] for c in _make(rng, idx_q, lengths, sym=len(alphabet))]
    cands += [[ord(c) for c in s] for s in ("hamming", "h香mmüng", "hammers", "ham", "")]
    corpus = rf.Corpus.from_u32_list([_chars(c) for c in cands])
    rows, lens = R.pad_rows(cands)
    queries = [q, [ord(c) for c in "hamming"], [ord(c) for c in "h香mmüng"], q[:10] + [0x4E2D] + q[10:]]  # the last one: a symbol the corpus does not hold
    for qq in queries:
        bc = MOD[metric].BatchComparator(_chars(qq))
        for label, args, pad in _variants(metric):
            for op in OPS:
                _eq(bc.many(op, corpus, args), R.ops(metric, op, qq, rows, lens, None, pad), f"chars {metric} {label} op {op}")
            _eq(bc.many(N.OP_DISTANCE, corpus, args, score_cutoff=6), R.ops(metric, N.OP_DISTANCE, qq, rows, lens, 6, pad), f"chars {metric} {label} cutoff")
            exp = R.ops(metric, N.OP_SIMILARITY, qq, rows, lens, 1, pad)
            idx, sc = bc.filter_many(N.OP_SIMILARITY, corpus, args, score_cutoff=1)
            assert idx.tolist() == R.keep(exp).tolist()
    if metric == "hamming":
        i = [_chars(c) for c in cands].index("h香mmüng")
        assert int(MOD[metric].BatchComparator("hamming").distance_many(corpus)[i]) == 2  # hamming.rs: diff_multibyte


@pytest.mark.parametrize("metric", R.METRICS)
def test_char_corpus_with_more_than_254_symbols_and_an_overflow_class_query_symbol(metric):
    rng = np.random.default_rng(32)
    common = list(range(0x400, 0x400 + 250))
    rare = list(range(0x3000, 0x3000 + 40))  # each of them once or twice in the corpus: the overflow class
    q = [common[i] for i in rng.integers(len(common), size=20)]
    q[3], q[17] = rare[5], rare[6]
    cands = []
    for i in range(400):
        L = int(rng.integers(0, 45)) if i % 3 else 20
        c = _near(rng, list(range(len(q))), L, 250, i % 4)  # positions of the query by index, noise as indices into `common`
        c = [q[v] if (v < len(q) and i % 2 == 0) else common[v % 250] for v in c]
        cands.append(c)
    for j, r in enumerate(rare):
        cands[j * 7][0:0] = [r]
    cands.append(list(q))
    cands.append(q[:3] + [rare[7]] + q[4:])  # differs from the query in ONE overflow-class symbol: the two must be told apart
    corpus = rf.Corpus.from_u32_list([_chars(c) for c in cands])
    own, lumped = corpus.alphabet_size()
    assert own == 254 and lumped >= 8  # the inputs: an overflow class exists
    rows, lens = R.pad_rows(cands)
    bc = MOD[metric].BatchComparator(_chars(q))
    for label, args, pad in _variants(metric):
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY):
            _eq(bc.many(op, corpus, args), R.ops(metric, op, q, rows, lens, None, pad), f"overflow {metric} {label} op {op}")
        exp = R.ops(metric, N.OP_DISTANCE, q, rows, lens, None, pad)
        order = _best_first(exp, R.keep(exp), N.OP_DISTANCE)[:5]
        scores, idx = bc.topk(corpus, 5, args=args)
        assert idx.tolist() == order
    raw = R.raw_many(metric, q, rows, lens)
    assert raw[-2] != raw[-1]  # the inputs: the overflow-class symbol decides


# ------------------------------------------------------------------------------------------------ several tiles per wavefront, in a child process
def test_several_tiles_per_wavefront():
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "compare_check.py")], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, RF_COMPARE_MAX_BLOCKS="1"))
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])  # one child, never retried
