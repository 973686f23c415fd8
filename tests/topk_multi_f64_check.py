"""Run by tests/test_gpu_topk_multi_f64.py in child processes with RF_TRACE_PLAN=1 (the library reads its switches once per process).

  multitile   with RF_SCAN_BLOCKS_PER_CU=1 and RF_TOPK_SAMPLE=8: the corpora of tests/topk_multi_check.py's mode of that name -- every wavefront of the
              fused kernel owns at least 3 tiles and the first one a fourth, partial one -- single-length and ragged; normalized Levenshtein with
              queries of 64 and 20 symbols, normalized Indel and the fuzz ratio, q = 4, k = 16, every row `==` the ranking of the oracle's float64
              scores.  The plan lines must show a fused group of 4 and a sample pass for every call: a loop over rf_topk_f64 would pass everything else.
  roads       default switches, a small corpus: which lists run fused (groups of 4 and 2) and which go per query, every row against the oracle
  roads_off   the same lists with RF_TOPK_MULTI=0: every query per query, the same rows

Exit status 0 = all as expected.  The plan lines go to stderr; this process reads its own through a pipe."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from oracle import oracle as o  # noqa: E402
from topk_multi_check import PlanLines, parse, plant, variants  # noqa: E402

ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
GPU = {"levenshtein": rf.distance.levenshtein.BatchComparator, "indel": rf.distance.indel.BatchComparator, "ratio": rf.fuzz.RatioBatchComparator,
       "jaro": rf.distance.jaro.BatchComparator, "jaro_winkler": rf.distance.jaro_winkler.BatchComparator, "osa": rf.distance.osa.BatchComparator,
       "damerau_levenshtein": rf.distance.damerau_levenshtein.BatchComparator}
ORA = {"levenshtein": o.levenshtein.BatchComparator, "indel": o.indel.BatchComparator, "ratio": o.fuzz.RatioBatchComparator, "jaro": o.jaro.BatchComparator,
       "jaro_winkler": o.jaro_winkler.BatchComparator, "osa": o.osa.BatchComparator}


def f64_lines(pl):
    return [parse(ln) for ln in pl.text.splitlines() if ln.startswith("[rf plan] topk_multi_f64:")]


def ranking(scores, k, desc):
    idx = np.nonzero(~np.isnan(scores))[0]
    v = scores[idx]
    order = np.lexsort((idx, -v if desc else v))[:k]
    return v[order], idx[order]


def oracle_scores(metric, q, op, host, ragged, indel_ratio=False, **kw):
    if metric == "ratio":
        ob, op = (o.indel.BatchComparator(q) if indel_ratio else o.fuzz.RatioBatchComparator(q)), NS
    else:
        ob = ORA[metric](q)
    return ob.rows(op, host, nthreads=8, **kw) if host is not None else ob.many(op, ragged[0], ragged[1], nthreads=8, **kw)


def rows_differ(got, metric, qs, op, k, host, ragged, **kw):
    bad = []
    for j, q in enumerate(qs):
        es, ei = ranking(oracle_scores(metric, q, op, host, ragged, **kw), k, op in (N.OP_SIMILARITY, NS))
        s, i = got[j]
        if s.dtype != np.float64 or len(s) != len(es) or not (s == es).all() or i.tolist() != ei.tolist():
            bad.append((j, list(zip(s.tolist(), i.tolist()))[:4], list(zip(es.tolist(), ei.tolist()))[:4]))
    return bad


def multitile():
    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1" and os.environ.get("RF_TOPK_SAMPLE") == "8", "run with RF_SCAN_BLOCKS_PER_CU=1 RF_TOPK_SAMPLE=8"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    waves = cus * 4
    n = (waves * 3 + 1) * 64 - 27
    print(f"{cus} CUs: {waves} wavefronts, {n} candidates = {-(-n // 64)} tiles", flush=True)
    rng = np.random.default_rng(20261019)
    q64, q20 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8)), bytes(rng.integers(97, 122, size=20, dtype=np.uint8))
    failures = 0
    for shape in ("rows", "ragged"):
        if shape == "rows":
            host = rng.integers(48, 122, size=(n, 64), dtype=np.uint8)

            def put(r, row):
                host[r] = np.resize(row, 64)

            plant(rng, put, n, variants(q64) + variants(q20), 4099)
            corpus, ragged = rf.Corpus.from_device_rows(torch.from_numpy(host).cuda()), None
            tiles = -(-n // 64)
        else:
            # lengths 0..64, the multiples of 16 and the queries' lengths more often than the rest: exact tiles of many lengths, a mixed section, tails of every size
            lens = np.where(rng.random(n) < 0.5, rng.choice([16, 20, 32, 48, 64], size=n), rng.integers(0, 65, size=n))
            for j, q in enumerate(variants(q64) + variants(q20)):
                lens[7 + 11 * j:: 4099] = len(q)
            offsets = np.zeros(n + 1, dtype=np.uint64)
            offsets[1:] = np.cumsum(lens)
            data = rng.integers(48, 122, size=int(offsets[-1]), dtype=np.uint8)

            def put(r, row):
                data[int(offsets[r]): int(offsets[r + 1])] = row

            plant(rng, put, n, variants(q64) + variants(q20), 4099)
            host, ragged = None, (data, offsets)
            corpus = rf.Corpus.from_ragged(data, offsets)
            tiles = corpus.slot_count // 64
        assert tiles >= waves * 3 + 1, (tiles, waves)
        for metric, base, op in (("levenshtein", q64, NS), ("levenshtein", q20, ND), ("indel", q64, NS), ("ratio", q20, N.OP_SIMILARITY)):
            qs = variants(base)
            cs = [GPU[metric](q) for q in qs]
            with PlanLines() as pl:
                got = GPU[metric].topk_multi(cs, corpus, 16, op)
            bad = rows_differ(got, metric, qs, op, 16, host, ragged)
            road = f64_lines(pl)
            if len(road) != 1 or road[0]["groups"] != [4] or road[0]["per_query"] != 0 or road[0]["sample"] != 1:
                bad.append(("road", pl.text[-500:]))
            print(f"{shape} {metric} len1={len(base)} op={op} x4 top-16: {'ok' if not bad else bad}", flush=True)
            failures += len(bad)
        del corpus
    print("FAILURES", failures)
    return failures


def roads(off):
    rng = np.random.default_rng(7)
    n = 64 * 6 + 9
    host = rng.integers(48, 122, size=(n, 64), dtype=np.uint8)
    q64 = bytes(rng.integers(48, 122, size=64, dtype=np.uint8))
    qs = variants(q64) + [q64[:20], q64[5:25]]

    def put(r, row):
        host[r] = np.resize(row, 64)

    plant(rng, put, n, qs, 53)
    corpus = rf.Corpus.from_rows(host)
    indel_ratio = rf.Args().ratio_indel_normalization()
    # name -> (metric, op, k, call keywords, oracle keywords, the fused groups and the per-query count the plan must name): 4 queries of 64 symbols + 2 of 20
    want = {
        "similarity": ("levenshtein", NS, 16, {}, {}, [4, 2], 0),
        "distance": ("levenshtein", ND, 16, {}, {}, [4, 2], 0),
        "indel": ("indel", NS, 16, {}, {}, [4, 2], 0),
        "ratio": ("ratio", N.OP_SIMILARITY, 16, {}, {}, [4, 2], 0),
        "ratio_indel": ("ratio", NS, 16, {"args": indel_ratio}, {"indel_ratio": True}, [4, 2], 0),
        "w222": ("levenshtein", NS, 16, {"weights": (2, 2, 2)}, {"weights": (2, 2, 2)}, [4, 2], 0),
        "w225": ("levenshtein", NS, 16, {"weights": (2, 2, 5)}, {"weights": (2, 2, 5)}, [4, 2], 0),
        "w000": ("levenshtein", ND, 16, {"weights": (0, 0, 0)}, {"weights": (0, 0, 0)}, [4, 2], 0),
        "w123": ("levenshtein", NS, 16, {"weights": (1, 2, 3)}, {"weights": (1, 2, 3)}, [], 6),
        "w1024": ("levenshtein", NS, 16, {"weights": (1024, 1024, 1024)}, {"weights": (1024, 1024, 1024)}, [], 6),  # maximum 1024 x 64 > 65535
        "loose": ("levenshtein", NS, 64, {"score_cutoff": 0.3}, {"score_cutoff": 0.3}, [4, 2], 0),
        "tight": ("levenshtein", NS, 16, {"score_cutoff": 0.9}, {"score_cutoff": 0.9}, [], 6),
        "k65": ("levenshtein", NS, 65, {}, {}, [], 6),
    }
    for name, (metric, op, k, call_kw, ora_kw, groups, per_query) in want.items():
        cs = [GPU[metric](q) for q in qs]
        with PlanLines() as pl:
            got = GPU[metric].topk_multi(cs, corpus, k, op, **call_kw)
        road = f64_lines(pl)
        assert len(road) == 1, (name, pl.text)
        if off:
            groups, per_query = [], 6
        assert road[0]["groups"] == groups and road[0]["per_query"] == per_query and road[0]["q"] == 6 and road[0]["k"] == k and road[0]["sample"] == 0, (name, road)
        bad = rows_differ(got, metric, qs, op, k, host, None, **ora_kw)
        assert not bad, (name, bad)
        if name == "loose":
            assert all(0 < len(s) < k for s, _ in got), name  # only the planted rows come that close: count < k on the fused road
        if name == "w000":
            assert all((s == 0.0).all() and i.tolist() == list(range(k)) for s, i in got), name
    # a mixed list: the two 64-symbol Levenshtein queries pair up, everything else goes per query
    members = [("levenshtein", qs[0]), ("jaro", qs[0]), ("osa", qs[1]), ("levenshtein", qs[1]), ("jaro_winkler", qs[4]), ("damerau_levenshtein", qs[5]), ("levenshtein", qs[4])]
    with PlanLines() as pl:
        got = GPU["levenshtein"].topk_multi([GPU[m](q) for m, q in members], corpus, 16, NS)
    road = f64_lines(pl)
    assert len(road) == 1 and road[0]["groups"] == ([] if off else [2]) and road[0]["per_query"] == (7 if off else 5), road
    for j, (m, q) in enumerate(members):
        if m != "damerau_levenshtein":  # (the oracle has none; tests/test_gpu_topk_multi_f64.py checks it against tests/dl_reference.py)
            assert not rows_differ([got[j]], m, [q], NS, 16, host, None), (m, j)
    print("roads_off ok" if off else "roads ok")
    return 0


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    mode = sys.argv[1]
    sys.exit(1 if (multitile() if mode == "multitile" else roads(mode == "roads_off")) else 0)
