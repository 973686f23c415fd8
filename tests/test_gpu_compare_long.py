"""hamming / prefix / postfix on the device (rf_compare.hip) at their length limits, BIT-exact against tests/compare_reference.py.  tests/test_gpu_compare.py
never leaves the first five chunk rows of a string; here: hamming's four-rows-in-flight loop over 1 .. 64 passes with every tail, postfix's backward walk at
every (len1 - len2) mod 16 both ways and from chunk row 17 on, the ballot early-out with one lane alive for thousands of symbols, the dynamic-LDS attribute on
either side of its edge (a query of 49 104 / 49 105 symbols), the query limit (150 000 answered, 150 001 refused with the output untouched), candidates of
65 535 symbols and more (the host packer), `char` corpora of 300 and 5000 symbols with an overflow class, all 256 byte values, every result road at 600,
49 105 and 150 000 symbols, a shuffled sequence of calls against fresh handles, and the pack-time layouts and the several-tiles-per-wavefront walk in child
processes (tests/compare_long_check.py).  The inputs are those of tests/compare_long_inputs.py; tests/test_compare_long_inputs.py holds them to their conditions
without a GPU, and every test here asserts the condition it stands on before it looks at a device value.

Every test runs all four ops, uncut and with cutoffs at an attained value and on either side of it, hamming strict and padded.  "By bits": f64 results are
compared as u64, so the None NaN and the Err NaN are different values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

import compare_long_check as K
import compare_long_inputs as L
import compare_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "compare_long_check.py")
# limits of the child processes: four times the wall time measured on an MI355X, rounded up to a whole 30 s (the factor is for a shared machine)
CHILD_LIMIT = {"multitile": 30, "layout": 30, "save": 30}  # measured, the whole test around each child: multitile 3.3 s, layout 2.4 .. 2.6 s, save 4.2 s


def _ok(bad):
    assert not bad, (len(bad), bad[:8])


def _lens(name):
    return np.array([len(c) for c in L.case(name).cands], dtype=np.int64)


def _child(mode, *argv, **env):
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT[mode]), sys.executable, CHECK, mode, *argv], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, **env))
    assert r.returncode == 0 and "FAILURES 0" in r.stdout, (r.returncode, r.stdout[-4000:], r.stderr[-2000:])  # one child, never retried


# ------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("qlen", L.QUERY_LENS)
def test_single_length_and_ragged_corpora(qlen):
    names = L.length_cases()[qlen]
    assert {int(v) for n in names[:3] for v in _lens(n)} == {qlen - 1, qlen, qlen + 1}
    lens = _lens(names[3])
    assert (lens == qlen).sum() >= 64 and (lens < qlen).any() and (lens > qlen).any()
    for name in names:
        _ok(K.parity(name, qlen))
    # hamming without pad: the Err encodings sit exactly on the lengths that differ
    bc = rf.distance.hamming.BatchComparator(L.case(names[3]).queries[qlen])
    corpus = K.corpus_of(names[3])
    differ = lens != qlen
    got = bc.many(N.OP_DISTANCE, corpus, score_cutoff=1)
    assert ((got == N.DIFFERENT_LENGTH_U32) == differ).all() and ((got == N.NONE_U32) <= ~differ).all()
    gotf = bc.many(N.OP_NORMALIZED_SIMILARITY, corpus, score_cutoff=0.9).view(np.uint64)
    assert ((gotf == N.DIFFERENT_LENGTH_F64_BITS) == differ).all() and ((gotf == N.NONE_F64_BITS) <= ~differ).all()
    assert not (bc.many(N.OP_DISTANCE, corpus, K.PAD) == N.DIFFERENT_LENGTH_U32).any()


def test_hamming_chunk_row_counts_the_lengths_above_do_not_reach():
    """7, 10, 11, 12 and 64 chunk rows: with them the tail of the unrolled loop runs with 2 and 3 rows after two passes (tests/compare_long_inputs.py)"""
    assert {L.nch(m) for m in L.HAMMING_EXTRA} == {7, 10, 11, 12, 64}
    assert {L.hamming_passes(m) for m in (160, 176)} == {(2, 2), (2, 3)}
    for m in L.HAMMING_EXTRA:
        _ok(K.parity(f"single-{m}-{m}", m))


@pytest.mark.parametrize("label", [230, 190, 23, 300])
def test_postfix_shifts_both_ways_and_from_chunk_row_17(label):
    lens = _lens("shift")
    if label == 230:
        assert {(230 - v) % 16 for v in L.SHIFT_LENGTHS} == set(range(16)) and lens.min() >= 200
    if label == 190:
        assert {(190 - v) % 16 for v in L.SHIFT_LENGTHS} == set(range(16)) and max(L.SHIFT_LENGTHS) > 190
    if label == 23:
        assert (lens == 300).sum() >= 64 and (300 - 23) // 16 >= 17 and (L.raw("shift", "postfix", 23)[lens == 300] > 0).sum() >= 5
    _ok(K.parity("shift", label))


def test_a_long_query_over_candidates_of_at_most_23_symbols():
    (q,) = L.case("mirror").queries
    assert q >= 300 and _lens("mirror").max() <= 23
    _ok(K.parity("mirror", q))


def test_one_lane_alive_through_4000_symbols_and_lanes_leaving_at_many_depths():
    for metric, t in (("prefix", 0), ("postfix", 1)):
        r = L.raw("earlyout", metric, 4100)[64 * t: 64 * t + 64]
        assert (r >= 4000).sum() == 1 and (r < 4).sum() == 63
    assert len(set((L.raw("earlyout", "prefix", 4100)[128:192] // 16).tolist())) >= 10
    corpus = K.corpus_of("earlyout")
    for metric, t, lane in (("prefix", 0, 37), ("postfix", 1, 5)):
        got = K.MOD[metric].BatchComparator(L.case("earlyout").queries[4100]).similarity_many(corpus)[64 * t: 64 * t + 64]
        assert got.tolist() == [4100 if i == lane else 0 for i in range(64)]
    _ok(K.parity("earlyout", 4100, corpus))


# ------------------------------------------------------------------------------------------------ the LDS edge
@pytest.mark.parametrize("qlen", [L.LDS_LAST_DEFAULT, L.LDS_FIRST_ATTRIBUTE])
def test_the_dynamic_lds_edge(qlen):
    """launch_compare_kind sets hipFuncAttributeMaxDynamicSharedMemorySize from (4 + ceil(len1 / 4) + 8) * 4 > 48 KiB on"""
    lds = (4 + (qlen + 3) // 4 + 8) * 4
    assert (lds > 48 << 10) == (qlen == L.LDS_FIRST_ATTRIBUTE) and (4 + (L.LDS_LAST_DEFAULT + 3) // 4 + 8) * 4 == 48 << 10
    name = f"ldslong-{qlen}"
    assert len(L.case(name).cands) == 67 and abs(_lens(name) - qlen).max() <= 100
    long_corpus, short_corpus = K.corpus_of(name), K.corpus_of("ldsshort")
    _ok(K.parity(name, qlen, long_corpus))
    _ok(K.parity("ldsshort", qlen, short_corpus))
    # a small launch after the large one: the same comparator classes, the same (NULL) stream
    _ok(K.parity("ldsshort", 23, short_corpus))
    _ok(K.parity(name, 23, long_corpus))


# ------------------------------------------------------------------------------------------------ the limit
def test_a_query_of_150000_symbols_is_answered():
    assert list(L.case("limit").queries) == [150_000] and len(L.case("limit").queries[150_000]) == 150_000
    _ok(K.parity("limit", 150_000))


SENTINEL32, SENTINEL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def _refused_everywhere(metric, q, corpus, path):
    """every entry point refuses the query with RF_ERR_UNSUPPORTED and writes nothing; -> the entry points tried"""
    lib = N.lib()
    bc = K.MOD[metric].BatchComparator(q)  # (the comparator itself exists: the refusal is plan()'s)
    n = len(corpus)
    a = N.RfArgs()
    lib.rf_args_default(C.byref(a))
    a.flags = N.FLAG_HAMMING_PAD
    hs = (C.c_void_p * 1)(bc._h)
    tried = []

    def refused(what, status, *buffers):
        tried.append(what)
        assert status == N.RF_ERR_UNSUPPORTED, (metric, what, status)
        assert "150 000" in lib.rf_last_error().decode()
        for b in buffers:
            assert (b == (SENTINEL32 if b.dtype == np.uint32 else SENTINEL64)).all(), (metric, what, "the output was written")

    def u32(m):
        return np.full(m, SENTINEL32, dtype=np.uint32)

    def u64(m):
        return np.full(m, SENTINEL64, dtype=np.uint64)  # (f64 outputs too: the sentinel is compared by bits)

    o = u32(n)
    refused("rf_many_u32", lib.rf_many_u32(bc._h, corpus._h, N.OP_DISTANCE, C.byref(a), o.ctypes.data, N.MEM_HOST, None), o)
    o = u64(n)
    refused("rf_many_f64", lib.rf_many_f64(bc._h, corpus._h, N.OP_NORMALIZED_SIMILARITY, C.byref(a), o.ctypes.data, N.MEM_HOST, None), o)
    o = u32(n)
    refused("rf_many_multi_u32", lib.rf_many_multi_u32(hs, 1, corpus._h, N.OP_SIMILARITY, C.byref(a), o.ctypes.data, N.MEM_HOST, None), o)
    o = u64(n)
    refused("rf_many_multi_f64", lib.rf_many_multi_f64(hs, 1, corpus._h, N.OP_NORMALIZED_DISTANCE, C.byref(a), o.ctypes.data, N.MEM_HOST, None), o)
    idx, sc, cnt = u64(n), u32(n), C.c_uint64(SENTINEL64)
    refused("rf_filter_u32", lib.rf_filter_u32(bc._h, corpus._h, N.OP_DISTANCE, C.byref(a), 0, n, idx.ctypes.data, sc.ctypes.data, C.byref(cnt), N.MEM_HOST, N.FILTER_BY_INDEX, None),
            idx, sc, np.array([cnt.value], dtype=np.uint64))
    idx, sc, cnt = u64(n), u64(n), C.c_uint64(SENTINEL64)
    refused("rf_filter_f64", lib.rf_filter_f64(bc._h, corpus._h, N.OP_NORMALIZED_DISTANCE, C.byref(a), 0, n, idx.ctypes.data, sc.ctypes.data, C.byref(cnt), N.MEM_HOST,
                                               N.FILTER_BY_SCORE, None), idx, sc, np.array([cnt.value], dtype=np.uint64))
    idx, sc, cnts = u64(n), u32(n), u64(1)
    refused("rf_filter_multi_u32", lib.rf_filter_multi_u32(hs, 1, corpus._h, N.OP_DISTANCE, C.byref(a), 0, n, idx.ctypes.data, sc.ctypes.data, cnts.ctypes.data, N.FILTER_BY_INDEX,
                                                           None), idx, sc, cnts)
    idx, sc, cnts = u64(n), u64(n), u64(1)
    refused("rf_filter_multi_f64", lib.rf_filter_multi_f64(hs, 1, corpus._h, N.OP_NORMALIZED_SIMILARITY, C.byref(a), 0, n, idx.ctypes.data, sc.ctypes.data, cnts.ctypes.data,
                                                           N.FILTER_BY_INDEX, None), idx, sc, cnts)
    sc, idx, cnt = u32(5), u64(5), C.c_uint32(SENTINEL32)
    refused("rf_topk_u32", lib.rf_topk_u32(bc._h, corpus._h, N.OP_DISTANCE, C.byref(a), 5, 0, sc.ctypes.data, idx.ctypes.data, C.byref(cnt), None, N.MEM_HOST, None), sc, idx,
            np.array([cnt.value], dtype=np.uint32))
    sc, idx, cnt = u64(5), u64(5), C.c_uint64(SENTINEL64)
    refused("rf_topk_f64", lib.rf_topk_f64(bc._h, corpus._h, N.OP_NORMALIZED_SIMILARITY, C.byref(a), 5, 0, sc.ctypes.data, idx.ctypes.data, C.byref(cnt), None, N.MEM_HOST, None),
            sc, idx, np.array([cnt.value], dtype=np.uint64))
    sc, idx, cnts = u32(5), u64(5), u32(1)
    refused("rf_topk_multi_u32", lib.rf_topk_multi_u32(hs, 1, corpus._h, N.OP_DISTANCE, C.byref(a), 5, 0, sc.ctypes.data, idx.ctypes.data, cnts.ctypes.data, None), sc, idx, cnts)
    sc, idx, cnts = u64(5), u64(5), u32(1)
    refused("rf_topk_multi_f64", lib.rf_topk_multi_f64(hs, 1, corpus._h, N.OP_NORMALIZED_DISTANCE, C.byref(a), 5, 0, sc.ctypes.data, idx.ctypes.data, cnts.ctypes.data, None),
            sc, idx, cnts)
    o = u32(n)
    refused("rf_stream_many_u32", lib.rf_stream_many_u32(bc._h, path.encode(), N.OP_DISTANCE, C.byref(a), o.ctypes.data, n, 8192, 0), o)
    o = u64(n)
    refused("rf_stream_many_f64", lib.rf_stream_many_f64(bc._h, path.encode(), N.OP_NORMALIZED_DISTANCE, C.byref(a), o.ctypes.data, n, 8192, 0), o)
    s = L.case("ldsshort").cands[0]
    buf = (C.c_uint8 * len(s)).from_buffer_copy(s.tobytes())
    v32, vf, some = C.c_uint32(SENTINEL32), C.c_uint64(SENTINEL64), C.c_int(-77)
    refused("rf_one_u32", lib.rf_one_u32(bc._h, buf, len(s), N.OP_DISTANCE, C.byref(a), 0, C.byref(v32), C.byref(some)), np.array([v32.value], dtype=np.uint32))
    assert some.value == -77
    refused("rf_one_f64", lib.rf_one_f64(bc._h, buf, len(s), N.OP_NORMALIZED_DISTANCE, C.byref(a), 0, C.cast(C.byref(vf), C.POINTER(C.c_double)), C.byref(some)),
            np.array([vf.value], dtype=np.uint64))
    assert some.value == -77
    import torch

    entries = torch.full((5, 2), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    st = lib.rf_topk_entries_device(bc._h, corpus._h, N.OP_DISTANCE, C.byref(a), 5, 0, entries.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    refused("rf_topk_entries_device", st)
    assert (entries.cpu().numpy() == -0x5A5A5A5A5A5A5A5B).all()
    # ... and from Python: RfError with that status
    for what, call in (("many", lambda: bc.many(N.OP_DISTANCE, corpus, K.PAD)), ("filter_many", lambda: bc.filter_many(N.OP_SIMILARITY, corpus, K.PAD, score_cutoff=1)),
                       ("topk", lambda: bc.topk(corpus, 5, args=K.PAD)), ("many_multi", lambda: type(bc).many_multi([bc], N.OP_DISTANCE, corpus, K.PAD)),
                       ("topk_multi", lambda: type(bc).topk_multi([bc], corpus, 5, args=K.PAD)),
                       ("filter_multi", lambda: type(bc).filter_multi([bc], N.OP_DISTANCE, corpus, K.PAD, score_cutoff=3)),
                       ("stream_many", lambda: bc.stream_many(N.OP_DISTANCE, path, args=K.PAD, segment_bytes=8192)), ("distance", lambda: bc.distance(s.tobytes(), K.PAD))):
        with pytest.raises(N.RfError) as e:
            call()
        assert e.value.status == N.RF_ERR_UNSUPPORTED, (metric, what, e.value)
    return tried


@pytest.mark.parametrize("metric", R.METRICS)
def test_a_query_of_150001_symbols_is_refused_on_every_entry_point_with_the_output_untouched(metric, tmp_path):
    q = np.concatenate([L.case("limit").queries[150_000], np.array([L.BASE], dtype=np.uint8)])
    assert len(q) == 150_001
    corpus = K.corpus_of("ldsshort")
    path = str(tmp_path / "short.rfc")
    corpus.save(path)
    tried = _refused_everywhere(metric, q, corpus, path)
    assert len(tried) == 17
    # the accepted side of the edge, through the same corpus: one symbol fewer is answered
    _ok(K.parity("ldsshort", L.LDS_FIRST_ATTRIBUTE, corpus, metrics=(metric,), ops=(N.OP_DISTANCE,)))
    got = K.MOD[metric].BatchComparator(q[:150_000]).many(N.OP_DISTANCE, corpus, K.PAD)
    _ok([] if not R.same_bits(got, R.ops(metric, N.OP_DISTANCE, q[:150_000], *L.rows_lens("ldsshort"), None, True)).size else ["150 000 symbols over the short corpus"])


# ------------------------------------------------------------------------------------------------ long candidates, char corpora, every byte value
@pytest.mark.parametrize("label", [23, 65_536])
def test_candidates_of_65535_symbols_and_more_among_short_ones(label):
    lens = _lens("longcand")
    assert {65_535, 65_536, 70_000} <= set(lens.tolist()) and (lens <= 66).sum() >= 190
    _ok(K.parity("longcand", label))


@pytest.mark.parametrize("name", ["char40-300", "char40-5000", "charover-300", "charover-5000"])
def test_char_corpora(name):
    c = L.case(name)
    held = set(np.concatenate(c.cands).tolist())
    assert c.wide and len(set(c.queries["absent"].tolist()) - held) == 1
    corpus = K.corpus_of(name)
    own, lumped = corpus.alphabet_size()
    if name.startswith("charover"):
        assert own == 254 and lumped == 36  # the inputs: an overflow class exists ...
        assert L.raw(name, "prefix", "main")[-3:].tolist() == [len(c.queries["main"]), 3, len(c.queries["main"]) - 4]  # ... and two of its symbols decide
    else:
        assert (own, lumped) == (40, 0)
    _ok(K.parity(name, "main", corpus))
    _ok(K.parity(name, "absent", corpus))
    _ok(K.selecting(name, "main", corpus, ks=(5,), orders=(N.FILTER_BY_INDEX,), slot_order=not name.startswith("charover")))


@pytest.mark.parametrize("length", [40, 300])
def test_all_256_byte_values(length):
    c = L.case(f"all256-{length}")
    assert set(np.concatenate(c.cands).tolist()) == set(range(256)) and {0x00, 0xFF} <= set(c.queries[length].tolist())
    corpus = K.corpus_of(c.name)
    _ok(K.parity(c.name, length, corpus))
    _ok(K.selecting(c.name, length, corpus, ks=(5,), orders=(N.FILTER_BY_INDEX,)))


# ------------------------------------------------------------------------------------------------ the roads
ROADS = [("road", 600, [0, 16, 600, L.LDS_FIRST_ATTRIBUTE]), (f"ldslong-{L.LDS_FIRST_ATTRIBUTE}", L.LDS_FIRST_ATTRIBUTE, [23, L.LDS_FIRST_ATTRIBUTE]), ("limit", 150_000, [150_000])]


def _rf_one(name, label, metric, rows):
    """rf_one_u32 / rf_one_f64 for candidates `rows` of the case: values, Some flags and the different-length error"""
    lib = N.lib()
    c = L.case(name)
    bc = K.MOD[metric].BatchComparator(c.queries[label])
    a = N.RfArgs()
    bad = []
    for vl, args, pad in K.variants(metric):
        for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 2), (N.OP_NORMALIZED_DISTANCE, 0.7), (N.OP_NORMALIZED_SIMILARITY, None)):
            exp = K.expected(name, label, metric, op, cutoff, pad)
            lib.rf_args_default(C.byref(a))
            a.flags = N.FLAG_HAMMING_PAD if pad else 0
            for i in rows:
                s = c.cands[i]
                buf = (C.c_uint8 * max(1, len(s))).from_buffer_copy(s.tobytes() or b"\0")
                some = C.c_int(-1)
                if op < 2:
                    a.cutoff_usize = N.NO_CUTOFF if cutoff is None else cutoff
                    v = C.c_uint32()
                    st = lib.rf_one_u32(bc._h, buf, len(s), op, C.byref(a), 0, C.byref(v), C.byref(some))
                    err, none, bits, want = exp[i] == N.DIFFERENT_LENGTH_U32, exp[i] == N.NONE_U32, v.value, int(exp[i])
                else:
                    a.cutoff_f64 = float("nan") if cutoff is None else cutoff
                    v = C.c_double()
                    st = lib.rf_one_f64(bc._h, buf, len(s), op, C.byref(a), 0, C.byref(v), C.byref(some))
                    e64 = int(exp[i: i + 1].view(np.uint64)[0])
                    err, none, bits, want = e64 == N.DIFFERENT_LENGTH_F64_BITS, e64 == N.NONE_F64_BITS, int(np.array([v.value]).view(np.uint64)[0]), e64
                if err:
                    ok = st == N.RF_ERR_INVALID_ARG and lib.rf_last_error().decode() == "Differing length arguments provided"
                else:
                    ok = st == N.RF_OK and some.value == (0 if none else 1) and (none or bits == want)
                if not ok:
                    bad.append(f"rf_one {name} query {label} {metric} {vl} op {op} cutoff {cutoff} candidate {i}: status {st} some {some.value} bits {bits:#x}, expected {want:#x}")
    return bad


@pytest.mark.parametrize("metric", R.METRICS)
@pytest.mark.parametrize("name,label,labels", ROADS, ids=["600", "49105", "150000"])
def test_every_road(name, label, labels, metric, tmp_path):
    import torch

    c = L.case(name)
    lens = _lens(name)
    n = len(c.cands)
    assert len(c.queries[label]) == label and (lens == label).sum() >= 64 and (lens != label).sum() >= 3  # hamming: candidates that are Err and candidates that are not
    corpus = K.corpus_of(name)
    m = (metric,)
    _ok(K.parity(name, label, corpus, metrics=m))  # many: host u32 and f64, the Err encodings exactly where the reference has them
    _ok(K.multi(name, labels, corpus, metrics=m))  # many_multi (Err-encoded), topk_multi, filter_multi
    _ok(K.selecting(name, label, corpus, metrics=m))  # filter_many in all three orders, topk k = 5 and 100 with ties by index, slot order
    q = c.queries[label]
    bc = K.MOD[metric].BatchComparator(q)
    path = str(tmp_path / "road.rfc")
    corpus.save(path)
    for vl, args, pad in K.variants(metric):
        # the Err encodings: exactly on the per-candidate roads, never on the selecting ones
        if metric == "hamming" and not pad:
            exp = K.expected(name, label, metric, N.OP_DISTANCE, None, pad)
            assert ((exp == N.DIFFERENT_LENGTH_U32) == (lens != label)).all()
            idx, _ = bc.filter_many(N.OP_DISTANCE, corpus, args)
            assert (lens[idx.astype(np.int64)] == label).all() and idx.size == (lens == label).sum()
            _, idx = bc.topk(corpus, 100, args=args)
            assert (lens[idx.astype(np.int64)] == label).all() and idx.size == min(100, (lens == label).sum())
        for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 2), (N.OP_NORMALIZED_DISTANCE, 0.7)):
            exp = K.expected(name, label, metric, op, cutoff, pad)
            bad = R.same_bits(bc.stream_many(op, path, args=args, score_cutoff=cutoff, segment_bytes=8192), exp)
            assert bad.size == 0, (metric, vl, op, cutoff, "stream_many", bad[:5])
            # the entries form follows topk's selection
            order = K.best_first(exp, R.keep(exp), op)[:5]
            entries = torch.empty((5, 2), dtype=torch.int64, device="cuda")
            bc.topk_entries_device(corpus, 5, entries, op=op, args=args, score_cutoff=cutoff)
            torch.cuda.synchronize()
            got = entries.cpu().numpy()
            assert got[: len(order), 1].tolist() == order and (got[len(order):] == -1).all(), (metric, vl, op, cutoff, got[:, 1], order)
    picks = [0, 1, n - 1] + [int(np.nonzero(lens != label)[0][0])]
    _ok(_rf_one(name, label, metric, picks))
    with pytest.raises(N.RfError, match="Differing length") if metric == "hamming" else _no_raise():
        bc.normalized_similarity(c.cands[picks[3]].tobytes())


class _no_raise:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


# ------------------------------------------------------------------------------------------------ the order of calls
def _order_calls():
    """about 40 calls over the "order" corpus, in a fixed shuffled order: (metric, query label, road, op, pad, cutoff)"""
    calls = []
    for label in (23, L.LDS_FIRST_ATTRIBUTE):
        for metric in R.METRICS:
            for vl, args, pad in K.variants(metric):
                calls += [(metric, label, "many", N.OP_DISTANCE, pad, None), (metric, label, "many", N.OP_NORMALIZED_SIMILARITY, pad, 0.5),
                          (metric, label, "filter", N.OP_SIMILARITY, pad, 1), (metric, label, "topk", N.OP_DISTANCE, pad, None),
                          (metric, label, "multi", N.OP_DISTANCE, pad, None)]
    rng = np.random.default_rng(20261019)
    return [calls[i] for i in rng.permutation(len(calls))]


def _run_call(call, corpus, comparators):
    metric, label, road, op, pad, cutoff = call
    bc = comparators[(metric, label)]
    args = K.PAD if pad else None
    if road == "many":  # (Err-encoded)
        return [bc.many(op, corpus, args, score_cutoff=cutoff)]
    if road == "filter":  # (plain None from here on)
        return list(bc.filter_many(op, corpus, args, score_cutoff=cutoff))
    if road == "topk":
        return list(bc.topk(corpus, 7, op=op, args=args, score_cutoff=cutoff))
    both = [comparators[(metric, 23)], comparators[(metric, L.LDS_FIRST_ATTRIBUTE)]]
    cls = type(bc)
    out = [cls.many_multi(both, op, corpus, args, score_cutoff=cutoff)]
    for pair in cls.topk_multi(both, corpus, 7, op=op, args=args, score_cutoff=cutoff) + cls.filter_multi(both, N.OP_SIMILARITY, corpus, args, score_cutoff=2):
        out += list(pair)
    return out


def test_no_result_depends_on_the_calls_before_it():
    c = L.case("order")
    lens = _lens("order")
    assert (lens == 23).sum() >= 64 and (lens == L.LDS_FIRST_ATTRIBUTE).sum() >= 2 and (lens <= 66).sum() >= 190
    calls = _order_calls()
    assert 38 <= len(calls) <= 42
    assert {(x[1], x[4]) for x in calls if x[0] == "hamming"} == {(23, False), (23, True), (L.LDS_FIRST_ATTRIBUTE, False), (L.LDS_FIRST_ATTRIBUTE, True)}
    assert {x[2] for x in calls} == {"many", "filter", "topk", "multi"}
    sizes = [x[1] for x in calls]
    assert sum(1 for a, b in zip(sizes, sizes[1:]) if a != b) >= 10  # the small launches and the large ones alternate
    corpus = K.corpus_of("order")
    shared = {(metric, label): K.MOD[metric].BatchComparator(c.queries[label]) for metric in R.METRICS for label in c.queries}
    got = [_run_call(call, corpus, shared) for call in calls]  # one corpus, one comparator per metric and query, one stream
    for call, res in zip(calls, got):
        fresh_corpus = K.corpus_of("order")
        fresh = {(call[0], label): K.MOD[call[0]].BatchComparator(c.queries[label]) for label in c.queries}
        exp = _run_call(call, fresh_corpus, fresh)
        assert len(exp) == len(res)
        for g, e in zip(res, exp):
            assert R.same_bits(np.asarray(g), np.asarray(e)).size == 0, call
    # ... and the fresh values are the reference's
    _ok(K.parity("order", 23, corpus) + K.parity("order", L.LDS_FIRST_ATTRIBUTE, corpus, ops=(N.OP_DISTANCE, N.OP_NORMALIZED_SIMILARITY)))


# ------------------------------------------------------------------------------------------------ pack-time layouts and several tiles per wavefront: child processes
@pytest.mark.parametrize("leg,env", [("no_mixed_host", {"RF_NO_MIXED_TILES": "1", "RF_DEVICE_PACK_MIN": "0"}), ("no_mixed_device", {"RF_NO_MIXED_TILES": "1", "RF_DEVICE_PACK_MIN": "1"}),
                                     ("no_rename", {"RF_NO_RENAME": "1"})])
def test_pack_time_layouts(leg, env):
    _child("layout", **env)


def test_a_corpus_file_saved_without_mixed_tiles(tmp_path):
    _child("save", str(tmp_path), RF_NO_MIXED_TILES="1", RF_DEVICE_PACK_MIN="0")
    corpora = {name: rf.Corpus.load(str(tmp_path / f"{name}.rfc")) for name, _ in K.LAYOUT_CASES}
    for name, _ in K.LAYOUT_CASES:
        assert len(corpora[name]) == len(L.case(name).cands)
    assert any(corpora[name].slot_count != K.corpus_of(name).slot_count for name, _ in K.LAYOUT_CASES)  # the inputs: a loaded layout is the saving process', not this one's own
    _ok(K.layout_checks(corpora))


def test_several_tiles_per_wavefront():
    _child("multitile", RF_COMPARE_MAX_BLOCKS="1")
