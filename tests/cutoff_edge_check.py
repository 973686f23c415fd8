"""Run by tests/test_gpu_cutoff_edges.py in child processes with RF_TRACE_PLAN=1 and each test id's switches (the library reads its switches once per process).

argv[1] is a leg of tests/cutoff_edge_inputs.py, or `multitile` (see ROADS) (its head says what the cutoff grid is and why the expected value is always the oracle called WITH the cutoff),
optionally `leg:i/m` for the i-th of m slices of the leg's (case, metric) pairs; argv[2] names the road the switches force, which must then show in the `[rf plan]` /
`[rf road]` lines of the process (ROADS below): a leg whose road was not reached fails.

For every (case, metric, op) of the leg the uncut vector is compared with the oracle and then, under EVERY cutoff of the grid, bit for bit as u64 patterns
(a None is a NaN: bits() below says which):
  many            into a host array, into a device tensor, in slot order (mapped back through slot_index())
  filter_many     by index and by score: the indices and values of the oracle's Somes
  topk            k = 16 under the cutoff: the oracle's Somes by (score, index)
and under the triples of the smallest, the largest, the threshold and the quotient values and of every fourth picked value, the fixed cutoffs and every cutoff under which some candidate's oracle answer differs from the filtered
uncut value (Jaro / Jaro-Winkler) also:
  topk            k = 1 and 300
  many_multi      four comparators: the query, the query with its last symbol replaced, the query again, the query without its last symbol
  topk_multi      the same four, k = 16, under the cutoff (the normalized ops of the usize metrics and the ratio: what the fused pass serves)
  filter_multi    the same four, for Jaro, Jaro-Winkler, OSA and the general weight table (tests/test_gpu_filter_multi_f64.py holds the fused metrics at exact values)
  stream_many     from the saved corpus in segments of 16 KiB (several segments)
  rf_one_f64      for the first and the last candidate and up to two of the candidates that differ
(a `char` corpus has neither a byte file nor rf_one_f64's byte candidates: the last two are left out there).

One line per case with the number of checks; a line per failing check; `ROADS` (what the trace showed), `SECONDS` and `FAILURES n` last; exit status 0 = all equal and
the road seen.  A mismatch is a value: the leg runs to its end.  A HIP error raises and ends the process.
"""
import ctypes as C
import os
import re
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# road name -> (the switches it needs, [(what must show, regular expression over the trace)], [(what must not show, regular expression)])
HEADS = {"RF_HEAD8_MIN": "1", "RF_RUN_MIN_TILES": "1", "RF_BAND_FILTER": "1"}
ROADS = {
    "default": ({}, [("a planned scan", r"^\[rf plan\] raw=")], []),
    "early": ({}, [("the early-out kernels", r"^\[rf plan\] raw=.* early=1 "), ("the streaming kernels under a cutoff", r"^\[rf plan\] raw=.* early=0 ")], []),
    "pack6": ({"RF_PACK6_MIN_TILES": "1"}, [("the 6-bit payload", r"^\[rf plan\] raw=.* data6=1")], []),
    "pack6-compiled": ({"RF_PACK6_MIN_TILES": "1", "RF_ASM_STREAM": "0"}, [("the 6-bit payload", r"^\[rf plan\] raw=.* data6=1")], []),
    "heads": (HEADS, [("the head plane", r"^\[rf plan\] raw=.* heads8=1 "), ("the band prefilter", r"^\[rf plan\] raw=.* head_need=[1-8] "),
                      ("the lane list", r"^\[rf road\] two-pass: lane list")], []),
    "heads-runs": (HEADS, [("the head plane", r"^\[rf plan\] raw=.* heads8=1 "), ("length-run views", r"^\[rf plan\] raw=.* by_runs=1 ")], []),
    "heads-tiles": (dict(HEADS, RF_LANE_COMPACT="0"), [("the head plane", r"^\[rf plan\] raw=.* heads8=1 "), ("the band prefilter", r"^\[rf plan\] raw=.* head_need=[1-8] "),
                                                      ("the tile list", r"^\[rf road\] two-pass: tile list")], [("the lane list", r"^\[rf road\] two-pass: lane list")]),
    "heads-nofilter": (dict(HEADS, RF_BAND_FILTER="0"), [("the head plane", r"^\[rf plan\] raw=.* heads8=1 ")], [("the band prefilter", r"^\[rf plan\] raw=.* head_need=[1-8] ")]),
    "compiled": ({"RF_ASM_STREAM": "0", "RF_ASM_CHUNK": "0"}, [("a planned scan", r"^\[rf plan\] raw=")], []),
    "jaro-priv": ({"RF_JARO_PRIV": "1"}, [("a planned scan", r"^\[rf plan\] raw=")], []),
    "multitile": ({"RF_SCAN_BLOCKS_PER_CU": "1", "RF_SCAN_BLOCKS_PER_CU_FULL": "1", "RF_SCAN_TILES_PER_WAVE": "2"},
                  [("the early-out kernels", r"^\[rf plan\] raw=.* early=1 "), ("the streaming kernels under a cutoff", r"^\[rf plan\] raw=.* early=0 ")], []),
}
# No trace line names an asm scan against its compiled twin, or the conflict-free table copy of the Jaro kernel: for `compiled`, `pack6-compiled` and `jaro-priv` the
# checker can only hold the switches themselves (asserted at start) and the values.  RF_JARO_PRIV changes a launch only where there is no cutoff (launch_jaro_word,
# rf_jaro.hip: the table epilogue), so the road `jaro-priv` compares the uncut vectors and nothing else: under a cutoff it would repeat the default ids.
# `multitile`: main() takes the cases of cutoff_edge_inputs.multitile_cases(CUs) instead of a leg's, and before a value is looked at asserts from the call's own
# `[rf plan]` line that the launch visits at least 2 x 4 x CUs tiles, i.e. that every wavefront owns two tiles or more; the result roads are many, filter_many by
# index and the top-16.
SWITCHES = sorted({k for env, _, _ in ROADS.values() for k in env} | {"RF_PACK6", "RF_HEAD6", "RF_STREAM", "RF_NO_RENAME", "RF_HEAD_TWO_PASS", "RF_FIRST_CHECK"})
NONE_BITS = 0x7FF8000000000000
PREFILL_BITS = 0xFFFFFFFFFFFFFFFF
SEGMENT = 16384

failures = 0
checks = 0
TRACE = None


def fail(line):
    global failures
    failures += 1
    if failures <= 60:
        print("FAIL " + line, flush=True)


class Trace:
    """this process' stderr (the library's trace lines) into a file that the checker reads at the end"""

    def __init__(self):
        sys.stderr.flush()
        self.real = os.dup(2)
        self.file = tempfile.TemporaryFile()
        os.dup2(self.file.fileno(), 2)
        self.at = 0

    def take(self):
        """what was written since the last take()"""
        sys.stderr.flush()
        self.file.seek(0, 2)
        end = self.file.tell()
        self.file.seek(self.at)
        text = self.file.read(end - self.at)
        self.at = end
        return text.decode("utf-8", "replace")

    def close(self):
        sys.stderr.flush()
        os.dup2(self.real, 2)
        self.file.seek(0)
        text = self.file.read().decode("utf-8", "replace")
        self.file.close()
        return text


def bits(v, device=False):
    """f64 -> u64 patterns with every None as NONE_BITS.  The oracle's None is whatever NaN numpy holds.  The device's None has exactly two patterns: the kernels
    store 0x7FF8000000000000, and the slots outside a cutoff's length window are pre-filled with all-ones words (launch_scan, rf_scan.hip: `a NaN, which is all
    "None" promises`; include/rfgpu.h: `a quiet NaN (test with isnan)`).  Any other NaN from the device -- one made by arithmetic, such as 0xFFF8000000000000, or
    hamming's different-length mark 0x7FF8000000000001 -- stays what it is and fails the compare."""
    v = np.ascontiguousarray(v, dtype=np.float64)
    u = v.view(np.uint64)
    none = ((u == np.uint64(NONE_BITS)) | (u == np.uint64(PREFILL_BITS))) if device else np.isnan(v)
    return np.where(none, np.uint64(NONE_BITS), u)


def multitile_least(case, cus):
    assert case.min_tiles >= 2 * 4 * cus, (case.min_tiles, cus)  # the corpus is what its sizing says
    return 2 * 4 * cus


def main(leg, road):
    import torch

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N

    import cutoff_edge_inputs as I

    global checks
    lib = N.lib()
    name, _, part = leg.partition(":")
    part_i, part_m = (int(x) for x in part.split("/")) if part else (0, 1)

    def same(what, got, exp):
        """`got` from the device (bit patterns as they are), `exp` from the oracle"""
        global checks
        checks += 1
        g, e = bits(got, device=True), bits(exp)
        if g.shape != e.shape:
            fail(f"{what}: {g.shape} values where {e.shape} are due")
            return
        bad = np.nonzero(g != e)[0]
        if len(bad):
            fail(f"{what}: {len(bad)} of {len(e)} differ, at {bad[:3].tolist()} got {np.asarray(got)[bad[:3]].tolist()} expected {np.asarray(exp)[bad[:3]].tolist()}")

    def pairs(what, got_idx, got_val, exp_idx, exp_val):
        global checks
        checks += 1
        if not (np.array_equal(np.asarray(got_idx, dtype=np.uint64), np.asarray(exp_idx, dtype=np.uint64)) and np.array_equal(bits(got_val, device=True), bits(exp_val))):
            fail(f"{what}: {len(got_idx)} entries, {len(exp_idx)} due; first {np.asarray(got_idx)[:3].tolist()} {np.asarray(got_val)[:3].tolist()} "
                 f"due {np.asarray(exp_idx)[:3].tolist()} {np.asarray(exp_val)[:3].tolist()}")

    def ordered(exp, op, by_score):
        """(indices, values) of the oracle's Somes: by index, or best first with ties by index"""
        idx = np.nonzero(~np.isnan(exp))[0]
        if by_score:
            v = exp[idx]
            idx = idx[np.lexsort((idx, v if I.is_distance(op) else -v))]
        return idx, exp[idx]

    def comparator(metric, q, wide):
        if metric.module == "ratio":
            return rf.fuzz.RatioBatchComparator(bytes(q))
        return getattr(rf.distance, metric.module).BatchComparator(q if wide else bytes(q))

    def arguments(metric):
        a = rf.Args()
        if "weights" in metric.kw:
            a = a.weights(metric.kw["weights"])
        if "prefix_weight" in metric.kw:
            a = a.prefix_weight(metric.kw["prefix_weight"])
        if metric.flags & I.FLAG_RATIO_INDEL_NORMALIZATION:
            a = a.ratio_indel_normalization()
        return a

    def one(bc, cand, op, args, cutoff):
        ca = args.score_cutoff(cutoff).to_c(True) if cutoff is not None else args.to_c(True)
        out, some = C.c_double(), C.c_int()
        buf = (C.c_uint8 * max(1, len(cand))).from_buffer_copy(bytes(cand) or b"\0")
        N.check(lib.rf_one_f64(bc._h, buf, len(cand), op, C.byref(ca), 0, C.byref(out), C.byref(some)))
        return np.array([out.value if some.value else np.nan])

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    trace = TRACE

    def enough_tiles(what, least):
        """multitile cases: the launch this call planned visits `least` tiles or more (or none at all: a cutoff nothing can pass) -- asserted, before its values are read"""
        lines = re.findall(r"^\[rf plan\] raw=.* tiles=\[(\d+),(\d+)\) of (\d+)", trace.take(), flags=re.M)
        assert lines and all(int(e) == int(b) or int(e) - int(b) >= least for b, e, _ in lines), (what, least, lines)

    pairs_done = -1
    for case in I.multitile_cases(cus) if name == "multitile" else I.leg_cases(name):
        t_case, checks0, failures0 = time.time(), checks, failures
        wide = case.device[0] == "chars"
        if wide:
            corpus, q_dev = rf.Corpus.from_u32_list(case.device[1]), case.device[2]
        elif case.device[0] == "rows":
            corpus, q_dev = rf.Corpus.from_device_rows(torch.from_numpy(case.device[1]).cuda()), case.q
        else:
            corpus, q_dev = rf.Corpus.from_ragged(case.device[1], case.device[2]), case.q
        n = len(corpus)
        slot_index = corpus.slot_index()
        real = slot_index != np.uint32(0xFFFFFFFF)
        if case.corpus[0] == "rows":
            cand_of = lambda i: case.corpus[1][i]  # noqa: E731
        else:
            cand_of = lambda i: case.corpus[1][int(case.corpus[2][i]):int(case.corpus[2][i + 1])]  # noqa: E731
        # the four queries of the multi-query roads (bytes for the oracle; the device's are the same symbols)
        alt = case.q.copy()
        if len(alt):
            alt[-1] = 126 if not wide else (alt[-1] - 48 + 1) % 40 + 48
        four = [case.q, alt, case.q, case.q[:-1]]
        if wide:
            symbols = I.chars()[2]
            four_dev = [I.to_str(symbols[x.astype(np.int64) - 48]) for x in four]
        else:
            four_dev = four
        path = None
        with tempfile.TemporaryDirectory() as tmp:
            if not wide and not case.min_tiles:
                path = os.path.join(tmp, "edges.rfc")
                corpus.save(path)
            for metric in case.metrics:
                pairs_done += 1
                if pairs_done % part_m != part_i:
                    continue
                args = arguments(metric)
                scorers = [I.Scorer(metric, x, case.corpus) for x in four]
                bcs = [comparator(metric, x, wide) for x in four_dev]
                sc, bc, cls = scorers[0], bcs[0], type(bcs[0])
                fused_topk = metric.family != "jaro" and metric.name not in ("osa", "levenshtein(2,2,3)")
                per_query_filter = not fused_topk
                for op in metric.ops:
                    what0 = f"{case.tag} {metric.name} {I.OP_NAMES[op]}"
                    cutoffs, kept, _ = I.cutoff_grid(sc, op, case.extra(metric, op), case.most)
                    full = sc(op)
                    same(f"{what0} no cutoff", bc.many(op, corpus, args), full)
                    if road == "jaro-priv":
                        continue
                    # the cutoffs of every road: the triples of must_values() (the smallest, the largest, the threshold and quotient values) and of every fourth
                    # picked value, and the fixed cutoffs
                    must = I.must_values(full, I.thresholds(metric, op), case.extra(metric, op))
                    sparse = {int(np.float64(c).view(np.uint64))
                              for c in [cutoffs[3 * p + t] for p in range(len(kept)) if p % 4 == 0 or kept[p] in must for t in range(3)] + cutoffs[3 * len(kept):]}
                    for c in cutoffs:
                        what = f"{what0} cutoff {c!r}"
                        exp = sc(op, c)
                        if case.min_tiles:
                            trace.take()
                            got = bc.many(op, corpus, args, score_cutoff=c)
                            enough_tiles(what, multitile_least(case, cus))
                            same(what + " many", got, exp)
                            idx, val = bc.filter_many(op, corpus, args, capacity=n, order=N.FILTER_BY_INDEX, score_cutoff=c)
                            pairs(what + " filter_many by index", idx, val, *ordered(exp, op, False))
                            best_i, best_v = ordered(exp, op, True)
                            s, i = bc.topk(corpus, 16, op, args, score_cutoff=c)
                            pairs(what + " topk 16", i, s, best_i[:16], best_v[:16])
                            continue
                        same(what + " many", bc.many(op, corpus, args, score_cutoff=c), exp)
                        out = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
                        bc.many(op, corpus, args, out=out, score_cutoff=c)
                        torch.cuda.synchronize()
                        same(what + " many (device tensor)", out.cpu().numpy(), exp)
                        slots = bc.many(op, corpus, args.slot_order(), score_cutoff=c)
                        back = np.empty(n, dtype=np.float64)
                        back[slot_index[real]] = slots[real]
                        same(what + " many (slot order)", back, exp)
                        for order, by_score in ((N.FILTER_BY_INDEX, False), (N.FILTER_BY_SCORE, True)):
                            idx, val = bc.filter_many(op, corpus, args, capacity=n, order=order, score_cutoff=c)
                            pairs(what + f" filter_many order {order}", idx, val, *ordered(exp, op, by_score))
                        best_i, best_v = ordered(exp, op, True)
                        s, i = bc.topk(corpus, 16, op, args, score_cutoff=c)
                        pairs(what + " topk 16", i, s, best_i[:16], best_v[:16])
                        flipped = np.nonzero(bits(exp) != bits(I.filtered(full, op, c)))[0][:2].tolist() if metric.family == "jaro" else []
                        if int(np.float64(c).view(np.uint64)) not in sparse and not flipped:
                            continue
                        for k in (1, 300):
                            s, i = bc.topk(corpus, k, op, args, score_cutoff=c)
                            pairs(what + f" topk {k}", i, s, best_i[:k], best_v[:k])
                        exps = [exp, scorers[1](op, c), exp, scorers[3](op, c)]
                        got = cls.many_multi(bcs, op, corpus, args, score_cutoff=c)
                        for j in range(4):
                            same(what + f" many_multi row {j}", got[j], exps[j])
                        if fused_topk:
                            for j, (s, i) in enumerate(cls.topk_multi(bcs, corpus, 16, op, args, score_cutoff=c)):
                                bi, bv = ordered(exps[j], op, True)
                                pairs(what + f" topk_multi row {j}", i, s, bi[:16], bv[:16])
                        if per_query_filter:
                            for j, (idx, val) in enumerate(cls.filter_multi(bcs, op, corpus, args, capacity=n, score_cutoff=c)):
                                pairs(what + f" filter_multi row {j}", idx, val, *ordered(exps[j], op, False))
                        if wide:
                            continue
                        same(what + " stream_many", bc.stream_many(op, path, None, args, segment_bytes=SEGMENT, score_cutoff=c), exp)
                        for i in [0, n - 1] + flipped:
                            same(what + f" rf_one_f64 candidate {i}", one(bc, cand_of(i), op, args, c), exp[i:i + 1])
        del corpus
        print(f"{case.tag}: {checks - checks0} checks, {failures - failures0} bad, {time.time() - t_case:.1f} s", flush=True)


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    leg, road = sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "default"
    env, must, must_not = ROADS[road]
    assert all(os.environ.get(k) == v for k, v in env.items()) and not [k for k in SWITCHES if k in os.environ and k not in env], f"road {road} runs with exactly {env}"
    t_start = time.time()
    TRACE = Trace()
    try:
        main(leg, road)
    finally:
        text = TRACE.close()
    seen = {what: len(re.findall(rx, text, flags=re.M)) for what, rx in must + must_not}
    print("ROADS", seen)
    for what, rx in must:
        if not seen[what]:
            fail(f"road {road}: {what} was never planned")
    for what, rx in must_not:
        if seen[what]:
            fail(f"road {road}: {what} was planned {seen[what]} times")
    if checks == 0:
        fail("nothing was checked")
    print(f"SECONDS {time.time() - t_start:.1f}")
    print("CHECKS", checks)
    print("FAILURES", failures)
    sys.exit(1 if failures else 0)
