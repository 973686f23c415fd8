"""The comparisons of tests/test_gpu_compare_long.py, and its child processes.  A helper and a program, not a test file.

As a module: `parity`, `selecting` and `multi` run one case of tests/compare_long_inputs.py on the device and return a list of differences from
tests/compare_reference.py, BY BITS (empty = equal).  As a program, started by the tests once per leg, because the library reads its switches once per process:

  compare_long_check.py multitile      with RF_COMPARE_MAX_BLOCKS=1: one workgroup, so four wavefronts walk every tile of the corpus.  "mtsingle" (1000-symbol
                                       candidates, 64 x 9 + 5) and "shift" (200..215 and 300 symbols, whole tiles plus leftovers): lengths, shifts and early-out state
                                       change from tile to tile along a wavefront's walk, and the one-live-lane tiles t = 0, 1 of the planted group come directly
                                       before the tiles t + 4 where every lane matches fully.  The host layout is held to that order first.
  compare_long_check.py layout         with RF_NO_MIXED_TILES=1 (RF_DEVICE_PACK_MIN=0: packed on the host, =1: on the device) or RF_NO_RENAME=1: the 256-symbol
                                       cases and the ragged 200..215 / 300 one through many, filter_many, topk and slot order
  compare_long_check.py save DIR       packs the same corpora under this process' switches and saves them to DIR/<case>.rfc (the parent loads them)

Exit status 0 = all equal.  Prints one line per (case, query, metric) so a failure names its kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402

import compare_long_inputs as L  # noqa: E402
import compare_reference as R  # noqa: E402

MOD = {"hamming": rf.distance.hamming, "prefix": rf.distance.prefix, "postfix": rf.distance.postfix}
OPS = (N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY)
PAD = rf.Args().pad()
LAYOUT_CASES = [("all256-40", 40), ("all256-300", 300), ("shift", 230)]


def variants(metric):
    """(label, Args or None, pad) -- hamming runs strict and padded"""
    return [("", None, False)] if metric != "hamming" else [("strict", None, False), ("pad", PAD, True)]


def corpus_of(name):
    c = L.case(name)
    return (rf.Corpus.from_u32_list if c.wide else rf.Corpus.from_list)(c.cands)


def expected(name, label, metric, op, cutoff, pad, query=None):
    rows, lens = L.rows_lens(name)
    q = L.case(name).queries[label] if query is None else query
    raw = L.raw(name, metric, label) if query is None else L.raw_of(name, metric, query)
    return R.ops(metric, op, q, rows, lens, cutoff, pad, raw)


def cutoffs(op, uncut):
    """an attained value and one on either side of it; for the normalized ops 0.0, 0.5, 1.0 and an attained score and its two neighbours"""
    some = uncut[R.keep(uncut)]
    if op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        if not some.size:
            return [0, 1]
        v = int(np.sort(some)[some.size // 2])
        return sorted({max(v - 1, 0), v, v + 1})
    cs = [0.0, 0.5, 1.0]
    if some.size:
        v = float(np.sort(some)[some.size // 2])
        cs += [float(np.nextafter(v, -1.0)), v, float(np.nextafter(v, 2.0))]
    return cs


def best_first(exp, some, op):
    desc = op in (N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY)
    return sorted(some.tolist(), key=lambda i: ((-float(exp[i]) if desc else float(exp[i])), i))


def _diff(got, exp, what, out):
    bad = R.same_bits(np.asarray(got), exp)
    if bad.size:
        out.append(f"{what}: {bad.size} differ, first at {bad[:4].tolist()}: got {np.asarray(got)[bad[:4]].tolist()}, expected {exp[bad[:4]].tolist()}")


def parity(name, label, corpus=None, metrics=R.METRICS, ops=OPS):
    """every op, uncut and at the cutoffs, through `many`"""
    out = []
    corpus = corpus_of(name) if corpus is None else corpus
    q = L.case(name).queries[label]
    for metric in metrics:
        bc = MOD[metric].BatchComparator(q)
        for vl, args, pad in variants(metric):
            for op in ops:
                uncut = expected(name, label, metric, op, None, pad)
                _diff(bc.many(op, corpus, args), uncut, f"{name} query {label} {metric} {vl} op {op}", out)
                for c in cutoffs(op, uncut):
                    _diff(bc.many(op, corpus, args, score_cutoff=c), expected(name, label, metric, op, c, pad), f"{name} query {label} {metric} {vl} op {op} cutoff {c}", out)
    return out


def road_cutoffs(op, uncut):
    some = uncut[R.keep(uncut)]
    if not some.size:
        return [None]
    if op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        return [None, int(np.sort(some)[some.size // 3])]
    return [None, float(np.sort(some)[some.size // 2])]


def selecting(name, label, corpus=None, metrics=R.METRICS, ks=(5, 100), orders=(N.FILTER_BY_INDEX, N.FILTER_BY_SCORE, N.FILTER_ANY), slot_order=True):
    """filter_many in its orders, topk with ties broken by index, and slot order: none of them returns an Err candidate.  (`slot_order` False: a u32 query
    with overflow-class symbols, for which include/rfgpu.h rules RF_FLAG_SLOT_ORDER out)"""
    out = []
    corpus = corpus_of(name) if corpus is None else corpus
    q = L.case(name).queries[label]
    n = len(L.case(name).cands)
    slots = corpus.slot_index()
    real = np.nonzero(slots != 0xFFFFFFFF)[0]
    if real.size != n:
        out.append(f"{name}: the slot index holds {real.size} candidates, not {n}")
    for metric in metrics:
        bc = MOD[metric].BatchComparator(q)
        for vl, args, pad in variants(metric):
            for op in OPS:
                for cutoff in road_cutoffs(op, expected(name, label, metric, op, None, pad)):
                    what = f"{name} query {label} {metric} {vl} op {op} cutoff {cutoff}"
                    exp = expected(name, label, metric, op, cutoff, pad)
                    some = R.keep(exp)
                    order = best_first(exp, some, op)
                    for o in orders:
                        idx, sc = bc.filter_many(op, corpus, args, score_cutoff=cutoff, order=o)
                        want = some.tolist() if o == N.FILTER_BY_INDEX else (order if o == N.FILTER_BY_SCORE else None)
                        if (idx.tolist() != want) if want is not None else (sorted(idx.tolist()) != some.tolist()):
                            out.append(f"filter order {o} {what}: indices {idx[:6].tolist()} ..., expected {(want or some.tolist())[:6]} ... ({idx.size} against {some.size})")
                        else:
                            _diff(sc, exp[idx.astype(np.int64)], f"filter order {o} {what}", out)
                        if bc.last_filter_count != some.size:
                            out.append(f"filter order {o} {what}: count {bc.last_filter_count}, expected {some.size}")
                    for k in ks:
                        scores, idx = bc.topk(corpus, k, op=op, args=args, score_cutoff=cutoff)
                        if idx.tolist() != order[:k]:
                            out.append(f"topk {k} {what}: indices {idx[:6].tolist()}, expected {order[:6]}")
                        else:
                            _diff(scores, exp[order[:k]], f"topk {k} {what}", out)
                    if not slot_order:
                        continue
                    got = bc.many(op, corpus, (args or rf.Args()).slot_order(), score_cutoff=cutoff)
                    if got.size != corpus.slot_count:
                        out.append(f"slot order {what}: {got.size} entries")
                    else:
                        _diff(got[real], exp[slots[real].astype(np.int64)], f"slot order {what}", out)
    return out


def multi(name, labels, corpus=None, metrics=R.METRICS, k=5):
    """many_multi, topk_multi and filter_multi over the queries `labels` of the case, in one call each"""
    out = []
    corpus = corpus_of(name) if corpus is None else corpus
    for metric in metrics:
        cls = MOD[metric].BatchComparator
        bcs = [cls(L.case(name).queries[lb]) for lb in labels]
        for vl, args, pad in variants(metric):
            for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_SIMILARITY, 3), (N.OP_NORMALIZED_DISTANCE, 0.8), (N.OP_NORMALIZED_SIMILARITY, None)):
                exps = [expected(name, lb, metric, op, cutoff, pad) for lb in labels]
                got = cls.many_multi(bcs, op, corpus, args, score_cutoff=cutoff)
                tk = cls.topk_multi(bcs, corpus, k, op=op, args=args, score_cutoff=cutoff)
                fm = cls.filter_multi(bcs, op, corpus, args, score_cutoff=cutoff, order=N.FILTER_BY_INDEX)
                for j, lb in enumerate(labels):
                    what = f"{name} {metric} {vl} query {lb} op {op} cutoff {cutoff}"
                    _diff(got[j], exps[j], f"many_multi {what}", out)  # (the Err encodings included)
                    some = R.keep(exps[j])
                    order = best_first(exps[j], some, op)[:k]
                    if tk[j][1].tolist() != order:
                        out.append(f"topk_multi {what}: indices {tk[j][1].tolist()}, expected {order}")
                    else:
                        _diff(tk[j][0], exps[j][order], f"topk_multi {what}", out)
                    if fm[j][0].tolist() != some.tolist():
                        out.append(f"filter_multi {what}: {fm[j][0].size} indices, expected {some.size}")
                    else:
                        _diff(fm[j][1], exps[j][some], f"filter_multi {what}", out)
    return out


def layout_checks(corpora=None):
    """what every layout leg runs: {case: Corpus} (None: packed here, under this process' switches)"""
    out = []
    for name, label in LAYOUT_CASES:
        corpus = corpus_of(name) if corpora is None else corpora[name]
        bad = parity(name, label, corpus, ops=(N.OP_DISTANCE, N.OP_NORMALIZED_SIMILARITY)) + selecting(name, label, corpus, ks=(5,), orders=(N.FILTER_BY_INDEX,))
        print(f"layout {name} query {label}: {'ok' if not bad else bad[:6]}", flush=True)
        out += bad
    return out


def _held_tiles(name, first_tile, n_tiles, first_cand):
    """the host layout keeps candidates first_cand .. as the whole tiles first_tile .., lane = position"""
    from rapidfuzz_rs_amd.corpus import host_layout, ragged

    lay = host_layout(*ragged(L.case(name).cands))
    if lay["identity"]:
        return
    for t in range(n_tiles):
        s0 = int(lay["tile_slot0"][first_tile + t])
        want = np.arange(first_cand + 64 * t, first_cand + 64 * t + 64)
        assert lay["orig"][s0: s0 + 64].tolist() == want.tolist(), (name, t, lay["orig"][s0: s0 + 64][:8])


def multitile():
    assert os.environ.get("RF_COMPARE_MAX_BLOCKS") == "1", "run with RF_COMPARE_MAX_BLOCKS=1"
    out = []
    # the planted group: "mtsingle" is a single-length corpus (tile t = candidates 64 t ..), "shift" keeps it as its exact tiles 32 .. 37 behind two tiles each of 200 .. 215
    assert len(L.case("mtsingle").cands) == 64 * 9 + 5
    _held_tiles("shift", 32, 6, 0)
    for name, labels in (("mtsingle", [1000]), ("shift", [300, 230, 190, 23])):
        corpus = corpus_of(name)
        for label in labels:
            for metric in R.METRICS:
                bad = parity(name, label, corpus, metrics=(metric,)) + selecting(name, label, corpus, metrics=(metric,), ks=(7,), orders=(N.FILTER_BY_INDEX,))
                print(f"multitile {name} query {label} {metric}: {'ok' if not bad else bad[:6]}", flush=True)
                out += bad
    return out


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "save":
        for name, _ in LAYOUT_CASES:
            corpus_of(name).save(os.path.join(sys.argv[2], f"{name}.rfc"))
        failures = []
    else:
        failures = {"multitile": multitile, "layout": layout_checks}[mode]()
    print("FAILURES", len(failures))
    sys.exit(1 if failures else 0)
