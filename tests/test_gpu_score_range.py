"""u32 scores at and above 2^31 on every result road, bit for bit against the CPU oracle (None positions included; for f64 the very doubles).

The device finishes every usize metric in 32-bit arithmetic mod 2^32 (tile_fin / usize_value in rf_device.hpp, the asm epilogues' unsigned multiply and compare)
and plan() refuses a call only when factor x (len1 + max_len) > 0xFFFFFFFE, so every score in [2^31, 0xFFFFFFFE] is a legal result.  One signed compare, one
`int` key half or one (int32_t) conversion to double -- in a scan, in may_pass() and the host-side length window, in normalize_kernel, in the filter's score
ordering, in the top-k selection and merge, or in the Python wrappers (torch.int32 device outputs viewed as uint32) -- would be invisible to every other test:
their largest u32 score is 2.0e9 < 2^31.

tests/score_range_inputs.py has the corpora, the values that are reachable and why (its module docstring), and the oracle's results, made once per process;
tests/test_score_range_inputs.py holds, without a GPU, that the corpora reach what they are here for.  The checker of the top-k roads, the selector and the
expected `out` vector are those of tests/topk_select_check.py.

  a  dense results: the four ops x every cutoff of the issue x (many to the host, to a torch.int32 and a torch.uint32 device tensor, many_multi with a second
     query, Args.slot_order() mapped back through corpus.slot_index()), per corpus x weight table
  b  thresholded results: filter_many by index and by score, into host and device arrays, with a capacity below the true count, index_base = 2^33 + 12345, and
     filter_multi of three queries
  c  top-k: k = 1, 16, 64 (in-scan lists) and 65, n, n + 7 (the selection, whose first digit now sits on bits 31..21), uncut and under the median cutoff;
     topk_keys_device (the 8-byte key score << 32 | index, with bit 63 set), topk_multi of three queries
  d  long_query() under (32767, 32767, 65534): the only place where a descending key 0xFFFFFFFF - s has s >= 2^31 (long_kernel, 516 words over ~33 000 columns)
  e  known answers at the very top, with no oracle, and the accept / refuse boundary of the common-factor roads at 0xFFFFFFFE
  f  the general table (65535, 65521, 65497) at its 31-bit boundary
  and the two ragged corpora once more after Corpus.save / Corpus.load.

Seconds per test id on an MI355X (also in DESIGN.md section 3): the short-query ids take 0.02 .. 0.12 s each, the whole module 21 s; a long_query() scan takes
0.74 s, so that leg has one id per op (0.74 s each) and one per k of its top-k (2.6 s: four roads, a scan each); the known answers of the 32 768-symbol query
take 4.7 s (ten scans of 512 words, six of them over one-candidate corpora)."""
import ctypes as C
import functools

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

import score_range_inputs as S
import topk_select_check as T

pytestmark = pytest.mark.gpu

LEV = rf.distance.levenshtein
OPS = {"distance": N.OP_DISTANCE, "similarity": N.OP_SIMILARITY, "normalized_distance": N.OP_NORMALIZED_DISTANCE, "normalized_similarity": N.OP_NORMALIZED_SIMILARITY}
FAMILY_IDS = ["uniform-ragged", "uniform-single", "indel65534-ragged", "indel65535-ragged"]
DISTANCE_CUTS = ("median", "2^31-1", "2^31", "0xFFFFFFFE", "0xFFFFFFFF", "2^32", "2^40", "0", "3f")
SIMILARITY_CUTS = ("0", "1", "median", "2^31", "0xFFFFFFFF", "2^32")
# (op, cutoff label) of the dense and the thresholded legs; None = no cutoff
DENSE_CALLS = ([(op, None) for op in OPS] + [("distance", c) for c in DISTANCE_CUTS] + [("similarity", c) for c in SIMILARITY_CUTS]
               + [(op, c) for op in ("normalized_distance", "normalized_similarity") for c in S.NORMALIZED_CUTOFFS])
FILTER_CALLS = [call for call in DENSE_CALLS if call[1] is not None]


def _call_id(call):
    return call[0] if call[1] is None else f"{call[0]}-cutoff-{call[1]}"


def _cutoff(name, weights, op, label):
    if label is None or isinstance(label, float):
        return label
    table = dict(zip(DISTANCE_CUTS, S.distance_cutoffs(name, weights))) if op == "distance" else dict(zip(SIMILARITY_CUTS, S.similarity_cutoffs(name, weights)))
    return table[label]


def _kw(weights, cutoff):
    return {"weights": weights} if cutoff is None else {"weights": weights, "score_cutoff": cutoff}


@functools.lru_cache(maxsize=None)
def _corpus(name):
    _, data, offsets = S.CORPORA[name]()
    return rf.Corpus.from_ragged(data, offsets)


def _none(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:8])


def _differs(what, got, exp, is_f):
    """[] or one line that names the first differing positions"""
    if got.shape != exp.shape:
        return [f"{what}: {got.shape} values for {exp.shape}"]
    wrong = np.nonzero(~T.same_scores(got, exp, is_f))[0]
    if not len(wrong):
        return []
    show = (lambda a: a[wrong[:3]].tolist()) if is_f else (lambda a: [hex(int(x)) for x in a[wrong[:3]]])
    return [f"{what}: differs at {len(wrong)} of {len(exp)}, first {wrong[:3].tolist()}: got {show(got)} want {show(exp)}"]


# ---------------------------------------------------------------------------------------------------------------- a. dense results
def _dense_forms(tag, name, corpus, weights, op, cutoff):
    """one (op, cutoff) through every output form of the dense calls"""
    import torch

    q = S.CORPORA[name]()[0]
    is_f = op >= N.OP_NORMALIZED_DISTANCE
    kw = _kw(weights, cutoff)
    exp = T.expected_out(S.scores(name, weights, op, cutoff), is_f)
    n = len(exp)
    bc = LEV.BatchComparator(q)
    bad = _differs(f"{tag} many -> host", bc.many(op, corpus, **kw), exp, is_f)
    # device `out`: a torch.int32 tensor (the bits of the uint32 scores) and a torch.uint32 one; float64 for the normalized ops.  4 entries of sentinel behind
    for dtype in (("float64",) if is_f else ("int32", "uint32")):
        if is_f:
            buf = torch.full((n + 4,), -7.0, dtype=torch.float64, device="cuda")
            out = buf
        else:
            buf = torch.full((n + 4,), T.SENTINEL32, dtype=torch.int32, device="cuda")
            out = buf.view(torch.uint32) if dtype == "uint32" else buf
            assert out.dtype == getattr(torch, dtype)
        assert bc.many(op, corpus, out=out, **kw) is out
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        host = host if is_f else host.view(np.uint32)
        bad += _differs(f"{tag} many -> torch.{dtype}", host[:n], exp, is_f)
        if not (host[n:] == (-7.0 if is_f else T.SENTINEL32)).all():
            bad.append(f"{tag} many -> torch.{dtype}: wrote behind the {n} scores")
    # many_multi: this query and a second one of 20 symbols
    q2 = S.second_query(name)
    both = LEV.BatchComparator.many_multi([bc, LEV.BatchComparator(q2)], op, corpus, **kw)
    bad += _differs(f"{tag} many_multi row 0", both[0], exp, is_f)
    bad += _differs(f"{tag} many_multi row 1", both[1], T.expected_out(S.scores_of(name, q2, weights, op, cutoff), is_f), is_f)
    # slot order, mapped back
    slots = bc.many(op, corpus, LEV.Args().slot_order(), **kw)
    index = corpus.slot_index()
    held = index != 0xFFFFFFFF
    if len(slots) != corpus.slot_count or sorted(index[held].tolist()) != list(range(n)):
        bad.append(f"{tag} slot order: {len(slots)} slots, {int(held.sum())} of them hold a candidate, for {n}")
    else:
        back = np.empty_like(exp)
        back[index[held]] = slots[held]
        bad += _differs(f"{tag} slot order", back, exp, is_f)
    return bad


@pytest.mark.parametrize("call", DENSE_CALLS, ids=_call_id)
@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_dense_results(name, weights, call):
    """every op and every cutoff of the issue through many (host, torch.int32, torch.uint32 / float64), many_multi and the slot order.  The maxima of the
    normalized ops, f x Mx and f x S, are themselves >= 2^31; `3f` is tight, so the head-plane and early-out roads see huge failing values behind a small
    cutoff; 2^32 and 2^40 are clamped to 0xFFFFFFFF by plan(), which the similarity side complements."""
    op = OPS[call[0]]
    cutoff = _cutoff(name, weights, call[0], call[1])
    if call == ("distance", "median"):
        assert cutoff >= S.BIT31
    _none(_dense_forms(f"{name} {weights} {_call_id(call)}", name, _corpus(name), weights, op, cutoff))


@pytest.mark.parametrize("name,weights", [S.SHORT_FAMILIES[0], S.SHORT_FAMILIES[2]], ids=[FAMILY_IDS[0], FAMILY_IDS[2]])
def test_dense_distance_after_save_and_load(name, weights, tmp_path):
    """a loaded corpus plans the same road: the dense distance, uncut and under the median cutoff"""
    path = str(tmp_path / "range.rfc")
    _corpus(name).save(path)
    corpus = rf.Corpus.load(path)
    q = S.CORPORA[name]()[0]
    bad = []
    for cutoff in (None, S.median_cutoff(name, weights)):
        got = LEV.BatchComparator(q).many(N.OP_DISTANCE, corpus, **_kw(weights, cutoff))
        bad += _differs(f"{name} loaded, cutoff {cutoff}", got, T.expected_out(S.scores(name, weights, N.OP_DISTANCE, cutoff), False), False)
    _none(bad)


# ---------------------------------------------------------------------------------------------------------------- b. thresholded results
def _listed(full, is_f, desc, by_score):
    """(scores, indices) a filter call returns: the oracle's Somes by ascending index, or best first with ties by ascending index"""
    if by_score:
        return T.select(full, len(full), desc, is_f)
    at = np.nonzero(T.valid_of(full, is_f))[0]
    return full[at], at.astype(np.uint64)


def _filter_roads(tag, bc, name, q, corpus, weights, op, cutoff):
    import torch

    is_f = op >= N.OP_NORMALIZED_DISTANCE
    kw = _kw(weights, cutoff)
    full = S.scores_of(name, q, weights, op, cutoff)
    n = len(full)
    bad = []
    for order, by_score in ((N.FILTER_BY_INDEX, False), (N.FILTER_BY_SCORE, True)):
        ev, ei = _listed(full, is_f, T.descending(op), by_score)
        ev = ev if is_f else ev.astype(np.uint32)
        ei = ei + np.uint64(T.BASE)
        for device_out in (False, True):
            idx, sc = bc.filter_many(op, corpus, capacity=n + 3, order=order, index_base=T.BASE, device_out=device_out, **kw)
            if device_out:
                torch.cuda.synchronize()
                idx, sc = idx.cpu().numpy().view(np.uint64), sc.cpu().numpy()
                sc = sc if is_f else sc.view(np.uint32)
            what = f"{tag} filter_many order {order} {'device' if device_out else 'host'} arrays"
            if bc.last_filter_count != len(ev):
                bad.append(f"{what}: count {bc.last_filter_count} for {len(ev)}")
            bad += _differs(what + " indices", idx, ei, False) or _differs(what + " scores", sc, ev, is_f)
        # a capacity below the true count: the count still true, the pairs valid, distinct and in the requested order among themselves
        cap = len(ev) // 2
        if cap:
            idx, sc = bc.filter_many(op, corpus, capacity=cap, order=order, index_base=T.BASE, **kw)
            what = f"{tag} filter_many order {order} capacity {cap} of {len(ev)}"
            place = {int(i): j for j, i in enumerate(ei.tolist())}
            at = [place.get(int(i), -1) for i in idx.tolist()]
            if bc.last_filter_count != len(ev) or len(idx) != cap:
                bad.append(f"{what}: count {bc.last_filter_count}, {len(idx)} pairs")
            elif min(at) < 0 or at != sorted(set(at)):
                bad.append(f"{what}: the indices are not distinct matches in the requested order: {idx[:4].tolist()}")
            else:
                bad += _differs(what + " scores", sc, ev[at], is_f)
    return bad


@pytest.mark.parametrize("call", FILTER_CALLS, ids=_call_id)
@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_thresholded_results(name, weights, call):
    """filter_many over the cutoffs of the dense legs: expected = numpy.nonzero of the oracle's vector, ordered by (score, index) for the by-score order"""
    op = OPS[call[0]]
    cutoff = _cutoff(name, weights, call[0], call[1])
    q = S.CORPORA[name]()[0]
    _none(_filter_roads(f"{name} {weights} {_call_id(call)}", LEV.BatchComparator(q), name, q, _corpus(name), weights, op, cutoff))


@pytest.mark.parametrize("call", [("distance", "median"), ("distance", "2^31"), ("distance", "3f"), ("similarity", "median"), ("normalized_distance", 0.5)], ids=_call_id)
@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_thresholded_results_of_three_queries(name, weights, call):
    """filter_multi of the corpus' query and two others, by index and by score: pair j is query j's filter_many, that is, the oracle's vector"""
    op = OPS[call[0]]
    is_f = op >= N.OP_NORMALIZED_DISTANCE
    cutoff = _cutoff(name, weights, call[0], call[1])
    qs = [S.CORPORA[name]()[0], S.second_query(name, 20), S.second_query(name, 33)]
    bcs = [LEV.BatchComparator(q) for q in qs]
    bad = []
    for order, by_score in ((N.FILTER_BY_INDEX, False), (N.FILTER_BY_SCORE, True)):
        rows = LEV.BatchComparator.filter_multi(bcs, op, _corpus(name), order=order, index_base=T.BASE, **_kw(weights, cutoff))
        for j, (idx, sc) in enumerate(rows):
            ev, ei = _listed(S.scores_of(name, qs[j], weights, op, cutoff), is_f, T.descending(op), by_score)
            what = f"{name} {weights} {_call_id(call)} filter_multi order {order} query {j}"
            if LEV.BatchComparator.last_filter_counts[j] != len(ev):
                bad.append(f"{what}: count {LEV.BatchComparator.last_filter_counts[j]} for {len(ev)}")
            bad += _differs(what + " indices", idx, ei + np.uint64(T.BASE), False) or _differs(what + " scores", sc, ev if is_f else ev.astype(np.uint32), is_f)
    _none(bad)


# ---------------------------------------------------------------------------------------------------------------- c. top-k
def _ks(n):
    return {"1": 1, "16": 16, "64": 64, "65": 65, "n": n, "n+7": n + 7}


@pytest.mark.parametrize("cut", [False, True], ids=["uncut", "median-cutoff"])
@pytest.mark.parametrize("k", ["1", "16", "64", "65", "n", "n+7"])
@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_topk_by_distance(name, weights, k, cut):
    """topk, topk with a host and a device `out`, and topk_entries_device, with index_base beyond 2^32.  k <= 64: the in-scan lists (WaveTopK, the 64-bit atomic
    minimum of the bounds) hold keys whose upper half has bit 31 set; k >= 65: the selection's first radix digit sits on bits 31..21."""
    cutoff = S.median_cutoff(name, weights) if cut else None
    full = S.scores(name, weights, N.OP_DISTANCE, cutoff)
    n = len(full)
    if k == "n" and not cut:
        ev, _ = T.select(full, n, False, False)
        assert len(ev) == n and int(ev[-1]) >= S.BIT31 and (name == "uniform_single_length" or int(ev[0]) < S.BIT31)  # the kept list itself crosses bit 31
    if cut:
        assert 4 * int((full == T.U64MAX).sum()) >= n
    q = S.CORPORA[name]()[0]
    _none(T.check_roads(f"{name} {weights} distance cutoff {cutoff}", LEV.BatchComparator(q), _corpus(name), N.OP_DISTANCE, _ks(n)[k], full, False, _kw(weights, cutoff)))


@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_topk_keys_device(name, weights):
    """the 8-byte keys score << 32 | index_base + index of rf_topk_keys_device with k = 16, uncut and under the median cutoff, and the scores of the same pass in a
    device `out`.  index_base = 0xFFFF0000 sets bit 31 of the lower half; on the single-length corpus every distance is >= 2^31, so every key has bit 63 set: a
    signed compare of keys, or of either half, would put them first or drop them."""
    import torch

    q = S.CORPORA[name]()[0]
    bc, corpus, k, base = LEV.BatchComparator(q), _corpus(name), 16, 0xFFFF0000
    bad = []
    for cutoff in (None, S.median_cutoff(name, weights)):
        full = S.scores(name, weights, N.OP_DISTANCE, cutoff)
        ev, ei = T.select(full, k, False, False)
        assert len(ev) == k
        want = [(int(s) << 32) | (base + int(i)) for s, i in zip(ev.tolist(), ei.tolist())]
        if name == "uniform_single_length":
            assert all(w >> 63 for w in want)  # (condition) bit 63 of every key
        keys = torch.full((k + 2,), T.SENTINEL64, dtype=torch.int64, device="cuda")
        out = torch.full((len(full) + 4,), T.SENTINEL32, dtype=torch.int32, device="cuda")
        bc.topk_keys_device(corpus, k, keys, N.OP_DISTANCE, index_base=base, out=out, **_kw(weights, cutoff))
        torch.cuda.synchronize()
        got = keys.cpu().numpy().view(np.uint64).tolist()
        if got[:k] != want or got[k:] != [T.SENTINEL64] * 2:
            at = next((j for j in range(k) if got[j] != want[j]), k)
            bad.append(f"{name} {weights} cutoff {cutoff}: keys differ at {at}: got {[hex(x) for x in got[at:at + 2]]} want {[hex(x) for x in want[at:at + 2]]}; tail {got[k:]}")
        host = out.cpu().numpy().view(np.uint32)
        bad += _differs(f"{name} {weights} cutoff {cutoff}: the scores of the same pass", host[:len(full)], T.expected_out(full, False), False)
    _none(bad)


@pytest.mark.parametrize("name,weights", S.SHORT_FAMILIES, ids=FAMILY_IDS)
def test_topk_of_three_queries(name, weights):
    """topk_multi of three queries equals the three single calls, and both equal the oracle's selection: k = 16 (fused in-scan lists) and k = 65"""
    qs = [S.CORPORA[name]()[0], S.second_query(name, 20), S.second_query(name, 33)]
    bcs = [LEV.BatchComparator(q) for q in qs]
    corpus = _corpus(name)
    bad = []
    for k in (16, 65):
        for cutoff in (None, S.median_cutoff(name, weights)):
            kw = _kw(weights, cutoff)
            rows = LEV.BatchComparator.topk_multi(bcs, corpus, k, N.OP_DISTANCE, index_base=T.BASE, **kw)
            for j, (s, i) in enumerate(rows):
                ev, ei = T.select(S.scores_of(name, qs[j], weights, N.OP_DISTANCE, cutoff), k, False, False)
                want = list(zip(ev.tolist(), (ei + np.uint64(T.BASE)).tolist()))
                s1, i1 = bcs[j].topk(corpus, k, N.OP_DISTANCE, index_base=T.BASE, **kw)
                for road, pairs in (("topk_multi", list(zip(s.tolist(), i.tolist()))), ("topk", list(zip(s1.tolist(), i1.tolist())))):
                    if pairs != want:
                        at = next((x for x, (g, w) in enumerate(zip(pairs, want)) if g != w), min(len(pairs), len(want)))
                        bad.append(f"{name} {weights} k={k} cutoff {cutoff} query {j} {road}: {len(pairs)} entries for {len(want)}, first at {at}: got {pairs[at:at + 2]} want {want[at:at + 2]}")
    _none(bad)


# ---------------------------------------------------------------------------------------------------------------- d. similarities >= 2^31
LONG_LEGS = ("similarity", "similarity-cutoff-2^31", "distance", "normalized_similarity", "topk-3", "topk-44")


@pytest.mark.parametrize("leg", LONG_LEGS)
def test_long_query_similarities_at_and_above_bit_31(leg):
    """A query of 33 000 symbols under (32767, 32767, 65534): the similarity 2 f lcs of its near-duplicates is >= 2^31, so a descending key 0xFFFFFFFF - s has
    s >= 2^31 here and nowhere else.  One leg per id: each scan is 516 words (65 sweeps) over about 33 000 columns."""
    name, weights = "long_query", S.W_INDEL_EVEN
    q = S.CORPORA[name]()[0]
    bc, corpus = LEV.BatchComparator(q), _corpus(name)
    sim = S.scores(name, weights, N.OP_SIMILARITY)
    above = int((sim >= S.BIT31).sum())
    assert above >= 30 and len(sim) - above >= 4  # (condition, also held in tests/test_score_range_inputs.py)
    if leg.startswith("topk"):
        k = int(leg[5:])
        _none(T.check_roads("long_query similarity", bc, corpus, N.OP_SIMILARITY, k, sim, False, {"weights": weights}))
        return
    op, cutoff = (N.OP_SIMILARITY, S.BIT31) if leg == "similarity-cutoff-2^31" else (OPS[leg], None)
    full = S.scores(name, weights, op, cutoff)
    if cutoff is not None:
        assert int((full != T.U64MAX).sum()) == above  # it keeps exactly the similarities with bit 31 set
    is_f = op >= N.OP_NORMALIZED_DISTANCE
    _none(_differs(f"long_query {leg}", bc.many(op, corpus, **_kw(weights, cutoff)), T.expected_out(full, is_f), is_f))


# ---------------------------------------------------------------------------------------------------------------- e. known answers at the very top
def _one_u32(bc, s2, op, weights, cutoff=None):
    """rf_one_u32 itself: (value, is_some)"""
    ca = LEV.Args().weights(weights)
    ca = (ca if cutoff is None else ca.score_cutoff(cutoff)).to_c(False)
    out, some = C.c_uint32(), C.c_int()
    buf = (C.c_uint8 * max(1, len(s2))).from_buffer_copy(s2 or b"\0")
    N.check(N.lib().rf_one_u32(bc._h, buf, len(s2), op, C.byref(ca), 0, C.byref(out), C.byref(some)))
    return out.value if some.value else None


def test_known_answers_of_a_32768_symbol_query():
    """"a" x 32768 under (32767, 32767, 65534): similarity 2 f lcs, distance f x (S - 2 lcs), S = 65 536; f x S = 0x7FFF0000"""
    f, w = 32767, S.W_INDEL_EVEN
    cands = [b"a" * 32768, b"b" * 32768, b"a" * 16384 + b"b" * 16384]
    assert [2 * f * 32768, 0, 2 * f * 16384] == [0x7FFF0000, 0, 0x3FFF8000]
    bc, corpus = LEV.BatchComparator(b"a" * 32768), rf.Corpus.from_list(cands)
    assert bc.similarity_many(corpus, weights=w).tolist() == [0x7FFF0000, 0, 0x3FFF8000]
    assert bc.distance_many(corpus, weights=w).tolist() == [0, 0x7FFF0000, 0x3FFF8000]
    assert bc.normalized_similarity_many(corpus, weights=w).tolist() == [1.0, 0.0, 0.5]
    assert [bc.distance(c, weights=w) for c in cands[1:]] == [0x7FFF0000, 0x3FFF8000]
    assert [_one_u32(bc, c, N.OP_SIMILARITY, w) for c in cands] == [0x7FFF0000, 0, 0x3FFF8000]


def test_largest_scores_and_the_refusal_boundary_of_the_indel_like_tables():
    """"c" x 48 over "d" x len2: no symbol in common, the distance is f x S itself, S = 48 + len2.  The first S with f x S > 0xFFFFFFFE is found by integer
    arithmetic: RF_ERR_UNSUPPORTED exactly from there on, a right answer one below -- 32767 x 131 076 = 0xFFFFFFFC, the largest score the device returns."""
    f, q = 32767, b"c" * 48
    first_refused = S.TOP // f + 1
    assert f * (first_refused - 1) <= S.TOP < f * first_refused and first_refused == 131_077
    bc = LEV.BatchComparator(q)
    for w in (S.W_INDEL_EVEN, S.W_INDEL_ODD):
        for total in (48 + S.INDEL_MAX_LEN, first_refused - 1):
            value = f * total
            assert S.BIT31 < value <= S.TOP and (total, value) in ((131_075, 0xFFFF7FFD), (131_076, 0xFFFFFFFC))
            cand = b"d" * (total - 48)
            corpus = rf.Corpus.from_list([cand])
            assert bc.distance_many(corpus, weights=w).tolist() == [value]
            assert bc.distance_many(corpus, weights=w, score_cutoff=value).tolist() == [value]
            assert bc.distance_many(corpus, weights=w, score_cutoff=S.TOP).tolist() == [value]
            assert bc.distance_many(corpus, weights=w, score_cutoff=value - 1).tolist() == [N.NONE_U32]
            assert bc.similarity_many(corpus, weights=w).tolist() == [0]
            assert bc.normalized_distance_many(corpus, weights=w).tolist() == [1.0]
            # the per-candidate methods return the same Python ints
            assert bc.distance(cand, weights=w) == value and bc.distance(cand, weights=w, score_cutoff=value - 1) is None
            assert _one_u32(bc, cand, N.OP_DISTANCE, w) == value and _one_u32(bc, cand, N.OP_DISTANCE, w, value) == value
            assert _one_u32(bc, cand, N.OP_DISTANCE, w, value - 1) is None
            s, i = bc.topk(corpus, 1, N.OP_DISTANCE, weights=w, index_base=T.BASE)
            assert (s.tolist(), i.tolist()) == ([value], [T.BASE])
        for total in (first_refused, first_refused + 1, first_refused + 4000):
            corpus = rf.Corpus.from_list([b"d" * (total - 48)])
            for call in (lambda: bc.distance_many(corpus, weights=w), lambda: bc.similarity_many(corpus, weights=w), lambda: bc.normalized_distance_many(corpus, weights=w),
                         lambda: bc.topk(corpus, 1, N.OP_DISTANCE, weights=w), lambda: bc.filter_many(N.OP_DISTANCE, corpus, weights=w, score_cutoff=5)):
                with pytest.raises(rf.RfError) as e:
                    call()
                assert e.value.status == N.RF_ERR_UNSUPPORTED, total


def test_largest_scores_and_the_refusal_boundary_of_uniform_weights():
    """65535 x 65 536 = 0xFFFF0000 is accepted and right, 65535 x 65 537 = 0xFFFFFFFF -- the image of None -- is refused"""
    f, w = 65535, S.W_UNIFORM
    first_refused = S.TOP // f + 1
    assert first_refused == 65_537 and f * 65_536 == 0xFFFF0000 and f * 65_537 == 0xFFFFFFFF
    for q in (b"c" * 48, b""):  # (with the empty query the distance is f x S itself; with "c" x 48 it is f x len2, every "c" substituted)
        bc = LEV.BatchComparator(q)
        len2 = first_refused - 1 - len(q)
        value = f * len2
        assert value > S.BIT31 and (len(q) or value == 0xFFFF0000)
        cand = b"d" * len2
        corpus = rf.Corpus.from_list([cand])
        assert bc.distance_many(corpus, weights=w).tolist() == [value]
        assert bc.distance_many(corpus, weights=w, score_cutoff=value).tolist() == [value]
        assert bc.distance_many(corpus, weights=w, score_cutoff=value - 1).tolist() == [N.NONE_U32]
        assert bc.similarity_many(corpus, weights=w).tolist() == [0]
        assert bc.distance(cand, weights=w) == value == _one_u32(bc, cand, N.OP_DISTANCE, w)
        for extra in (1, 2):
            with pytest.raises(rf.RfError) as e:
                bc.distance_many(rf.Corpus.from_list([b"d" * (len2 + extra)]), weights=w)
            assert e.value.status == N.RF_ERR_UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------- f. the general table
def test_general_table_at_its_31_bit_boundary():
    """(65535, 65521, 65497), a query of 40 symbols over 150 candidates of up to 32 768 - 40: worst = 32 768 x 65535 = 2^31 - 32 768 is accepted; the four ops
    and the distance under the median cutoff against the oracle; one candidate of 32 769 - 40 symbols more and the call is refused"""
    name, w = "general_boundary", S.W_GENERAL
    q, data, offsets = S.CORPORA[name]()
    bc, corpus = LEV.BatchComparator(q), _corpus(name)
    dist = S.scores(name, w, N.OP_DISTANCE)
    assert int(dist.max()) >> 30 == 1  # (condition) a distance with bit 30 set
    bad = []
    for opname, op in OPS.items():
        is_f = op >= N.OP_NORMALIZED_DISTANCE
        bad += _differs(f"general table {opname}", bc.many(op, corpus, weights=w), T.expected_out(S.scores(name, w, op), is_f), is_f)
    median = S.median_cutoff(name, w)
    bad += _differs("general table distance under the median cutoff", bc.distance_many(corpus, weights=w, score_cutoff=median),
                    T.expected_out(S.scores(name, w, N.OP_DISTANCE, median), False), False)
    _none(bad)
    cands = [data[int(offsets[i]): int(offsets[i + 1])].tobytes() for i in range(len(offsets) - 1)] + [b"x" * (32_769 - 40)]
    with pytest.raises(rf.RfError) as e:
        bc.distance_many(rf.Corpus.from_list(cands), weights=w)
    assert e.value.status == N.RF_ERR_UNSUPPORTED
