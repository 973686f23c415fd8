"""Run by tests/test_gpu_parity.py::test_scan_grid_kernels_many_tiles_per_wavefront in a subprocess with RF_SCAN_BLOCKS_PER_CU=1.

Every kernel is a grid-stride loop over tiles of 64 candidates, and what runs BETWEEN two tiles of one wavefront -- re-arming the per-lane state, re-initialising
an LDS row or a global scratch strip, resetting the column counter, a carry strip the previous tile left behind -- runs only from the second tile on.
RF_SCAN_BLOCKS_PER_CU_FULL (tests/multitile_check.py, tests/band_check.py) shrinks scan_grid_full() only.  Everything launched on scan_grid() =
min(ceil(tiles / 4), CUs x RF_SCAN_BLOCKS_PER_CU) -- the row-DP kernels of rf_damerau.hip and rf_long.hip, long_kernel and jaro_long_kernel on p.long_grid, the
cutoff early-out scans, the band kernels on band_grid_of() -- owns a second tile per wavefront only beyond CUs x 32 x 4 tiles (2.1 M candidates on 256 CUs) by
default.  With one workgroup per CU and the corpora sized here from the device's CU count and the launch's wavefronts per workgroup, every wavefront of the launch
under test walks at least 4 tiles (the arithmetic is held on the host by tests/test_scan_grid.py, not by the kernels).

argv[1] is the mode, so that a failure names its kernel; one line per kernel and shape with the candidate count and the tiles per wavefront; `FAILURES n` last;
exit status 0 = all equal.  A mismatch is a value: the mode runs to its end.  A HIP error raises and ends the process.

  damerau  dl_reg_kernel<16|32|64>, dl_kernel<DlCell8|DlCell16> in LDS (4 and 1 wavefronts per workgroup) and on the global strip, against tests/dl_reference.py.
           The reference is numpy and slow: each corpus draws its rows, with repetition, from a pool of a few hundred distinct rows (random rows and planted
           near-duplicates, the generator of tests/test_gpu_damerau.py); the reference runs once per pool row and a candidate expects ref[pool index].  The draw is
           random, so neighbouring tiles and lanes differ: a lane that inherits state from the previous tile inherits a wrong one.
  weights  wf_reg_kernel<16|32|64>, wf_kernel in LDS and on the global strip (RF_WF_REG=0 in a second child: wf_kernel for the short queries too), oracle.
  long     long_kernel<LEV|LCS|OSA> for queries of 513 / 1024 / 1500 symbols, jaro_long_kernel, oracle.  launch_jaro starts jaro_long_kernel once over the exact
           tiles and once over the views of the mixed section: the ragged Jaro corpora hold whole tiles of 16 lengths (the exact section alone gives every
           wavefront its 4) and a mixed tail of 37 candidates; the figure printed is that of the exact tiles.
  mixed    scan_kernel_mixed (rf_mixed.hip): a ragged corpus of at most RF_JOINT_MAX_TILES (16384) exact tiles, scanned without a length window by a query of at
           most 512 symbols, goes through ONE joint launch over the exact and the mixed tiles on scan_grid(exact + mixed) (launch_scan, rf_scan.hip).  Levenshtein,
           OSA, LCS and Indel, a query of 24 symbols (the 32-bit states) and one of 100 (the multi-word states), without a cutoff and under one too loose to
           leave a length out.
  cutoff   the default roads of the cutoff scans (early-out scans, the band kernels, the band pass of the hinted scan, filter_many, topk), oracle, with quirk
           Q8's excuse as test_gpu_parity._check_many has it.  The figure printed is that of the first pass, which runs on scan_grid() / band_grid_of().

The launches that walk a list of survivors are not this file's: sparse_lean_kernel and sparse_words_kernel (rf_sparse.hip), the head plane's listing pass and its
second pass over a tile list (rf_scan.hip), band_sparse_kernel.  Since list_max_grid() (rf_scan.hip) the knob caps their grids as well -- the second passes of the
cutoff mode here run on the capped grids too -- but several units per wavefront there is a matter of SURVIVOR counts, and tests/multitile_lists_check.py sizes
corpora for that, one mode per launch.  The hint kernels (rf_hint.hip) take scan_grid(units) with `units` survivors.

Seconds per mode, measured once on an MI355X (256 CUs: 262 117 candidates per corpus at 4 wavefronts per workgroup, 131 045 at 2, 65 509 at 1; the bucketed
corpus of query 64 has 488 861, the ragged Jaro corpora 262 181): MEASURED_SECONDS below; the timeouts of the test are about three times these, and at least 60 s.
"""
import os
import sys
import time

import numpy as np

MEASURED_SECONDS = {"damerau": 14, "weights": 31, "weights-lds": 9, "long": 17, "mixed": 3, "cutoff": 8}  # whole child process, wall clock
TILES_PER_WAVE = 4  # the floor; the candidate counts follow from it
LDS_BUDGET = 150 << 10  # plan() (rf_api_scan.hip): of the 160 KiB a gfx950 workgroup may hold


# ---------------------------------------------------------------------------------------------- the grid arithmetic (no GPU; tests/test_scan_grid.py reads these)
def candidates_for(cus, waves):
    """candidates of a corpus whose every wavefront owns >= TILES_PER_WAVE tiles on a grid of at most `cus` workgroups of `waves` wavefronts; the last tile is partial"""
    return 64 * TILES_PER_WAVE * waves * cus - 27


def tiles_per_wavefront(n_tiles, cus, waves, per_cu=1):
    """the fewest tiles a wavefront of scan_grid(n_tiles) workgroups x `waves` owns: wavefront w takes tiles w, w + stride, ..."""
    grid = max(1, min((n_tiles + 3) // 4, cus * per_cu))
    return n_tiles // (grid * waves)


def dl_waves(len1, longest):
    """wavefronts per workgroup of the damerau_levenshtein launch (plan(): dl_wide, dl_reg, wf_waves, wf_global)"""
    wide = max(len1, longest) > 254
    if not wide and len1 <= 64:
        return 4  # dl_reg_kernel
    row_bytes = max(len1, 1) * 64 * (8 if wide else 4)
    if row_bytes + len1 + 16 > LDS_BUDGET:
        return 4  # the global strip
    return min(4, (LDS_BUDGET - len1 - 16) // row_bytes)


def wf_waves(len1, reg=True):
    """wavefronts per workgroup of the general-weights Levenshtein launch"""
    if reg and len1 <= 64:
        return 4  # wf_reg_kernel
    row_bytes = (len1 + 1) * 64 * 4
    if row_bytes + len1 + 8 > LDS_BUDGET:
        return 4  # the global strip
    return min(4, (LDS_BUDGET - len1 - 8) // row_bytes)


DL_SHAPES = [  # (query length, longest candidate, what the plan must be)
    (16, 64, "reg16"), (17, 64, "reg32"), (32, 64, "reg32"), (33, 64, "reg64"), (64, 64, "reg64"),
    (100, 100, "lds8 x4"), (64, 300, "lds16 x4"), (256, 120, "lds16 x1"), (700, 64, "global16"),
]
WF_QUERIES = [16, 32, 64, 200, 700]


JARO_LENGTHS = 16  # distinct lengths of a ragged Jaro corpus, each in whole tiles


def jaro_exact_tiles(cus):
    """exact tiles of a ragged Jaro corpus: JARO_LENGTHS runs of equal size, together >= TILES_PER_WAVE x 4 wavefronts x cus"""
    return JARO_LENGTHS * -(-TILES_PER_WAVE * 4 * cus // JARO_LENGTHS)


def derived_sizes(cus):
    """every (CUs, wavefronts per workgroup, candidates) this checker sizes a corpus by"""
    out = {(cus, dl_waves(q, longest), candidates_for(cus, dl_waves(q, longest))) for q, longest, _ in DL_SHAPES}
    out |= {(cus, wf_waves(q, reg), candidates_for(cus, wf_waves(q, reg))) for q in WF_QUERIES for reg in (True, False)}
    out.add((cus, 4, candidates_for(cus, 4)))  # long, mixed, cutoff
    out.add((cus, 4, 64 * jaro_exact_tiles(cus)))  # the exact section of the ragged Jaro corpora
    return sorted(out)


# ---------------------------------------------------------------------------------------------- the checker
failures = 0
ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)


def report(tag, n, tpw, bad):
    global failures
    assert tpw >= TILES_PER_WAVE, (tag, n, tpw)  # the condition of this file, before any value is looked at
    print(f"{tag}: n={n} tiles/wavefront>={tpw} {'ok' if not bad else bad}", flush=True)
    failures += len(bad)


def ragged_from_lens(rng, lens):
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    return ALNUM[rng.integers(0, 62, size=int(offsets[-1]), dtype=np.uint8)], offsets


def plant_query(rng, data, offsets, q, every):
    """every `every`-th candidate: the query cut (or repeated) to the candidate's length, with 0..3 substitutions"""
    qa = np.frombuffer(q, dtype=np.uint8)
    for r in range(0, len(offsets) - 1, every):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if b - a >= 4:
            row = np.resize(qa, b - a).copy()
            row[rng.integers(0, b - a, size=r % 4)] = 122
            data[a:b] = row


def main(mode):
    global failures
    import torch

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N
    from rapidfuzz_rs_amd.utils import synth
    from oracle import oracle as o

    import dl_reference as R
    import test_gpu_damerau as TD
    import test_gpu_filter as TF
    import test_gpu_parity as TP

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print(f"mode {mode}: {cus} CUs, RF_SCAN_BLOCKS_PER_CU=1: scan_grid() <= {cus} workgroups", flush=True)

    def uniform_corpus(host):
        return rf.Corpus.from_device_rows(torch.from_numpy(host).cuda())

    def tpw_of(corpus, waves, tiles=None):
        return tiles_per_wavefront((corpus.slot_count + 63) // 64 if tiles is None else tiles, cus, waves)

    def oracle_check(tag, metric, q, data, offsets, corpus, waves, cases, tiles=None):
        """cases: (op name, kwargs); every value through test_gpu_parity._check_many (oracle, quirks Q2 / Q8)"""
        bad = []
        for op, kw in cases:
            try:
                TP._check_many(metric, q, data, offsets, op, corpus=corpus, **kw)
            except AssertionError as e:
                bad.append((op, kw, str(e)[:300]))
        n_tiles = (corpus.slot_count + 63) // 64 if tiles is None else tiles
        report(f"{tag} {metric}", len(corpus), tiles_per_wavefront(n_tiles, cus, waves), bad)

    if mode == "damerau":
        DL = rf.distance.damerau_levenshtein
        sym = 62
        for qlen, longest, plan in DL_SHAPES:
            waves = dl_waves(qlen, longest)
            assert (plan.endswith("x1") and waves == 1) or (not plan.endswith("x1") and waves == 4), (qlen, longest, plan, waves)
            n = candidates_for(cus, waves)
            rng = np.random.default_rng(7000 + qlen + longest)
            q = TD._rand(rng, qlen, sym)
            qv = [48 + v for v in q]
            bc = DL.BatchComparator(bytes(qv))
            pool_n = 4096 if qlen <= 64 and longest <= 64 else {100: 2048, 64: 1024, 256: 512, 700: 384}[qlen]

            def planted_row(top):
                """_planted on the query's head, the rest of the query behind it: the four swap-and-insert edits land inside the first `top` symbols,
                so that cutting the row there does not cut them off"""
                h = max(2, min(qlen, top) - 4)
                return TD._planted(rng, q[:h], sym, clip=1 << 30) + q[h:]

            for kind in ("single", "ragged"):
                # the pool: 3/4 random rows, 1/4 planted near-duplicates, in the length law of the corpus
                extra = None  # (the one long candidate of the "lds16 x4" shape: its own reference, not a pool row)
                if kind == "single":
                    L = 255 if longest == 300 else (96 if longest > 64 else 64)  # (255: the shortest row with 16-bit fields under a query of 64)
                    L = 48 if qlen == 700 else L
                    lens_of = lambda: L  # noqa: E731
                    top = L
                else:
                    top = 64 if longest == 300 else longest
                    lens_of = lambda: int(rng.integers(0, top + 1))  # noqa: E731
                    if longest == 300:
                        extra = (planted_row(64) + TD._rand(rng, 300, sym))[:300]
                pool = []
                planted = []
                for i in range(pool_n):
                    ln = lens_of()
                    if i % 4 == 0:
                        c = (planted_row(top) + TD._rand(rng, top, sym))[:ln] if kind == "single" else planted_row(top)[:top]
                        planted.append(c)
                    else:
                        c = TD._rand(rng, ln, sym)
                    pool.append(c)
                if kind == "ragged":
                    pool[1], pool[2] = [], []  # zero-length rows, whatever the draw
                # a condition on the INPUTS, from the restatement alone, for every shape: these rows tell this metric from OSA
                assert TD._frac_below_osa(q, planted[:40]) >= 0.5, (qlen, kind)
                rows, lens = R.pad_rows([[48 + v for v in c] for c in pool])
                t0 = time.time()
                dist = R.dl_many(qv, rows, lens)
                # the corpus: every pool row at least once, then the draw; shuffled
                pick = np.concatenate([np.arange(pool_n), rng.integers(0, pool_n, size=n - pool_n - (extra is not None))])
                rng.shuffle(pick)
                if kind == "single":
                    host = np.ascontiguousarray(rows[pick].astype(np.uint8))
                    corpus = uniform_corpus(host)
                    at_extra = None
                else:
                    at_extra = None if extra is None else int(rng.integers(0, len(pick)))
                    cl = lens[pick]
                    width = rows.shape[1]
                    mask = np.arange(width)[None, :] < cl[:, None]
                    data = rows.astype(np.uint8)[pick][mask]
                    if extra is not None:
                        off = int(cl[:at_extra].sum())
                        data = np.concatenate([data[:off], np.array([48 + v for v in extra], dtype=np.uint8), data[off:]])
                        cl = np.insert(cl, at_extra, 300)
                    offsets = np.zeros(len(cl) + 1, dtype=np.uint64)
                    offsets[1:] = np.cumsum(cl)
                    corpus = rf.Corpus.from_ragged(data, offsets)
                assert len(corpus) == n
                if extra is not None:
                    erows, elens = R.pad_rows([[48 + v for v in extra]])
                    edist = R.dl_many(qv, erows, elens)
                med = int(np.median(dist))
                bad = []
                for op, cutoff in ((N.OP_DISTANCE, None), (N.OP_NORMALIZED_SIMILARITY, None), (N.OP_DISTANCE, med)):
                    exp = R.ops(op, qv, rows, lens, cutoff, dist)[pick]
                    if extra is not None:
                        exp = np.insert(exp, at_extra, R.ops(op, qv, erows, elens, cutoff, edist)[0])
                    got = bc.many(op, corpus, score_cutoff=cutoff)
                    miss = _same(got, exp)
                    if len(miss):
                        bad.append((op, cutoff, len(miss), miss[:4].tolist(), got[miss[:4]].tolist(), exp[miss[:4]].tolist()))
                report(f"damerau {plan} query={qlen} {kind} (pool {pool_n}, reference {time.time() - t0:.1f} s)", n, tpw_of(corpus, waves), bad)
                del corpus

    elif mode == "weights":
        reg = os.environ.get("RF_WF_REG", "1") != "0"
        rng = np.random.default_rng(20261017)
        for qlen in WF_QUERIES if reg else [16, 32, 64]:
            waves = wf_waves(qlen, reg)
            n = candidates_for(cus, waves)
            q = synth.query(qlen, 555 + qlen)
            L = 24 if qlen <= 64 else (32 if qlen == 200 else 12)
            for kind in ("single", "ragged"):
                if kind == "single":
                    host = ALNUM[rng.integers(0, 62, size=(n, L), dtype=np.uint8)]
                    data, offsets = host.reshape(-1), np.arange(0, (n + 1) * L, L, dtype=np.uint64)
                    data = data.copy()
                    plant_query(rng, data, offsets, q, 13)
                    corpus = uniform_corpus(np.ascontiguousarray(data.reshape(n, L)))
                else:
                    data, offsets = ragged_from_lens(rng, rng.integers(0, L + L // 2 + 1, size=n))
                    plant_query(rng, data, offsets, q, 13)
                    corpus = rf.Corpus.from_ragged(data, offsets)
                dcut = 25 if qlen <= 64 else 2 * qlen
                for w in ((1, 2, 3), (3, 1, 2), (7, 11, 13)):
                    cases = [(op, {"weights": w}) for op in TP.OPS]
                    cases += [("distance", {"weights": w, "score_cutoff": dcut}), ("similarity", {"weights": w, "score_cutoff": 10}),
                              ("normalized_distance", {"weights": w, "score_cutoff": 0.4 if qlen <= 64 else 0.9}),
                              ("normalized_similarity", {"weights": w, "score_cutoff": 0.5 if qlen <= 64 else 0.1})]
                    oracle_check(f"weights {w} {'wf_reg' if reg and qlen <= 64 else 'wf'} x{waves} query={qlen} {kind}", "levenshtein", q, data, offsets, corpus, waves, cases)
                del corpus

    elif mode == "long":
        rng = np.random.default_rng(20261018)
        n = candidates_for(cus, 4)
        # single-length rows of 80 symbols; ragged: long runs of exact tiles of very different lengths (a wavefront's next tile after a 700-symbol one may hold
        # 3 symbols: fewer chunks than the strip still holds), and every length 0..200 for the mixed section and the short runs
        host = ALNUM[rng.integers(0, 62, size=(n, 80), dtype=np.uint8)]
        lens = np.where(rng.random(n) < 0.5, rng.choice([3, 30, 90, 330, 700], size=n), rng.integers(0, 201, size=n))
        rdata, roffsets = ragged_from_lens(rng, lens)
        for qlen in (513, 1024, 1500):
            q = synth.query(qlen, 0x10E6 + qlen)
            for kind in ("single", "ragged"):
                if kind == "single":
                    data, offsets = host.reshape(-1).copy(), np.arange(0, (n + 1) * 80, 80, dtype=np.uint64)
                    plant_query(rng, data, offsets, q, 97)
                    corpus = uniform_corpus(np.ascontiguousarray(data.reshape(n, 80)))
                else:
                    data, offsets = rdata.copy(), roffsets
                    plant_query(rng, data, offsets, q, 97)
                    corpus = rf.Corpus.from_ragged(data, offsets)
                for metric in ("levenshtein", "indel", "lcs_seq", "osa"):
                    cases = [("distance", {}), ("normalized_similarity", {})] + ([("similarity", {})] if qlen == 1024 else [])
                    oracle_check(f"long_kernel query={qlen} {kind}", metric, q, data, offsets, corpus, 4, cases)
                del corpus
        del host, rdata
        # jaro_long_kernel: every tile takes the flag strips (a query beyond 512 symbols, or candidates that stay beyond 512 after the window truncation)
        for qlen, lo, hi in ((600, 520, 760), (40, 1050, 1200)):
            q = synth.query(qlen, 0x1A20 + qlen)
            for kind in ("single", "ragged"):
                if kind == "single":
                    L = 700 if qlen == 600 else 1200
                    host = ALNUM[rng.integers(0, 62, size=(n, L), dtype=np.uint8)]
                    data, offsets = host.reshape(-1), np.arange(0, (n + 1) * L, L, dtype=np.uint64)
                    plant_query(rng, data, offsets, q, 97)
                    corpus = uniform_corpus(host)
                else:
                    # launch_jaro walks the exact tiles and the views of the mixed section in launches of their own: whole tiles of JARO_LENGTHS lengths across
                    # the range (neighbouring runs differ by 10..16 symbols, the first and the last by the whole range), so that the exact launch alone gives
                    # every wavefront its 4, and 37 leftovers of other lengths for the mixed section; shuffled
                    run_lens = np.linspace(lo, hi, JARO_LENGTHS).astype(np.int64)
                    per_run = 64 * (jaro_exact_tiles(cus) // JARO_LENGTHS)
                    lens = np.concatenate([np.repeat(run_lens, per_run), run_lens[0] + 1 + np.arange(37) % 7])
                    rng.shuffle(lens)
                    data, offsets = ragged_from_lens(rng, lens)
                    plant_query(rng, data, offsets, q, 97)
                    corpus = rf.Corpus.from_ragged(data, offsets)
                    launch_tiles = int(sum(np.count_nonzero(lens == L) // 64 for L in np.unique(lens)))  # the exact section, from the lengths alone
                    assert launch_tiles == jaro_exact_tiles(cus)
                kw = {} if kind == "single" else {"tiles": launch_tiles}
                oracle_check(f"jaro_long_kernel query={qlen} {kind}", "jaro", q, data, offsets, corpus, 4, [("similarity", {})], **kw)
                oracle_check(f"jaro_long_kernel query={qlen} {kind}", "jaro_winkler", q, data, offsets, corpus, 4, [("similarity", {}), ("distance", {})], **kw)
                del corpus, data

    elif mode == "mixed":
        rng = np.random.default_rng(20261019)
        n = candidates_for(cus, 4)
        lens = rng.integers(0, 41, size=n)  # every length 0..40: long runs of exact tiles, and the leftovers of each in the mixed section
        exact = int(sum(np.count_nonzero(lens == L) // 64 for L in range(41)))
        assert exact <= 16384 and exact * 64 < n  # one joint launch (RF_JOINT_MAX_TILES), and a mixed section
        for qlen in (24, 100):
            q = synth.query(qlen, 0x3D1 + qlen)
            data, offsets = ragged_from_lens(rng, lens)
            plant_query(rng, data, offsets, q, 13)
            corpus = rf.Corpus.from_ragged(data, offsets)
            assert exact < corpus.slot_count // 64
            for metric in ("levenshtein", "osa", "lcs_seq", "indel"):
                loose = 2 * (qlen + 40)  # no distance is beyond it and no length outside its window: the launch stays the joint one
                oracle_check(f"scan_kernel_mixed joint launch query={qlen} ragged", metric, q, data, offsets, corpus, 4,
                             [("distance", {}), ("normalized_similarity", {}), ("distance", {"score_cutoff": loose}), ("normalized_similarity", {"score_cutoff": 0.0})])
            del corpus

    elif mode == "cutoff":
        n = candidates_for(cus, 4)
        # (at these sizes, below RF_HEAD8_MIN = 16384 tiles, the cutoff scans are the general early-out kernels and the band kernels, one launch per scan)
        for qlen, cutoffs in ((64, (3, 8)), (256, (8, 31))):
            q = synth.query(qlen, 0xC070 + qlen)
            for kind in ("single", "bucketed"):
                if kind == "single":
                    rows = TF._band_rows(n, qlen, q, 0.01, seed=qlen)
                    data, offsets = rows.reshape(-1), np.arange(0, (n + 1) * qlen, qlen, dtype=np.uint64)
                    corpus = uniform_corpus(rows)
                    window_tiles = {k: (n + 63) // 64 for k in cutoffs}
                else:
                    # lengths qlen - 6 .. qlen + 6: a distance cutoff k leaves the 2 * min(k, 6) + 1 lengths within k of the query's; their whole tiles alone must
                    # give every wavefront its 4 (counted below from the lengths, a lower bound: leftovers and the sparse lengths add tiles)
                    in_window = 2 * min(min(cutoffs), 6) + 1
                    per_length = -(-n // in_window) + 64
                    data, offsets = TF._bucketed_long_corpus(q, seed=qlen, per_length=per_length, share=0.01)
                    corpus = rf.Corpus.from_ragged(data, offsets)
                    cl = np.diff(offsets.astype(np.int64))
                    window_tiles = {k: int(sum(np.count_nonzero(cl == L) // 64 for L in range(qlen - k, qlen + k + 1))) for k in cutoffs}
                for metric in ("levenshtein", "osa", "indel", "lcs_seq"):
                    for k in cutoffs:
                        # (Indel counts a substitution as 2: its window of lengths is the same, |len1 - len2| <= k)
                        oracle_check(f"cutoff scan query={qlen} {kind} distance<={k}", metric, q, data, offsets, corpus, 4, [("distance", {"score_cutoff": k})], tiles=window_tiles[k])
                    if qlen == 256:
                        oracle_check(f"cutoff scan query={qlen} {kind} normalized_similarity>=0.9", metric, q, data, offsets, corpus, 4,
                                     [("normalized_similarity", {"score_cutoff": 0.9})], tiles=window_tiles[min(cutoffs)])
                # filter_many and the top-16 under the cutoff
                bc, ob = rf.distance.levenshtein.BatchComparator(q), o.levenshtein.BatchComparator(q)
                k = cutoffs[1]
                exp = ob.many(N.OP_DISTANCE, data, offsets, nthreads=8, score_cutoff=k)
                idx_e, val_e = TF._some(exp)
                bad = []
                idx, val = bc.filter_many(N.OP_DISTANCE, corpus, score_cutoff=k)
                if not (np.array_equal(idx, idx_e) and np.array_equal(val, val_e)):
                    bad.append(("filter_many", len(idx), len(idx_e)))
                order = np.lexsort((idx_e, val_e))[:16]
                s, i = bc.topk(corpus, 16, score_cutoff=k)
                if list(zip(s.tolist(), i.tolist())) != [(int(val_e[j]), int(idx_e[j])) for j in order]:
                    bad.append(("topk16", list(zip(s.tolist(), i.tolist()))[:4], [(int(val_e[j]), int(idx_e[j])) for j in order][:4]))
                report(f"filter_many + topk16 query={qlen} {kind} distance<={k}", len(corpus), tiles_per_wavefront(window_tiles[k], cus, 4), bad)
                del corpus
        # the hinted scan on a near-duplicate corpus, twice: its first pass is the band launch on band_grid_of(), which the figure describes; the list that pass
        # leaves is walked on grids of its own (see the head of this file)
        q = synth.query(256, 0x4157 + 256)
        rows = TF._band_rows(n, 256, q, 0.75, seed=256 + 750, kinds=6)
        corpus = uniform_corpus(rows)
        bc, ob = rf.distance.levenshtein.BatchComparator(q), o.levenshtein.BatchComparator(q)
        exp = TF._u32(ob.rows(N.OP_DISTANCE, rows, nthreads=8))
        bad = []
        for rep in range(2):
            got = bc.distance_many(corpus, score_hint=16)
            miss = np.nonzero(got != exp)[0]
            if len(miss):
                bad.append((rep, len(miss), miss[:4].tolist(), got[miss[:4]].tolist(), exp[miss[:4]].tolist()))
        report("band pass of score_hint=16 query=256 single near-duplicates, two calls", n, tpw_of(corpus, 4), bad)
        del corpus
        # the early-out Jaro launch (a similarity cutoff of 0.9 or more takes scan_grid())
        q = synth.query(64, 0xC070 + 64)
        rows = TF._band_rows(n, 64, q, 0.01, seed=64)
        data, offsets = rows.reshape(-1), np.arange(0, (n + 1) * 64, 64, dtype=np.uint64)
        corpus = uniform_corpus(rows)
        oracle_check("early-out jaro query=64 single similarity>=0.9", "jaro_winkler", q, data, offsets, corpus, 4, [("similarity", {"score_cutoff": 0.9})])
        oracle_check("early-out jaro query=64 single similarity>=0.9", "jaro", q, data, offsets, corpus, 4, [("similarity", {"score_cutoff": 0.9})])
    else:
        raise SystemExit(f"unknown mode {mode!r}")


def _same(got, exp):
    if got.dtype == np.uint32:
        return np.nonzero(got != exp)[0]
    return np.nonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[0]


if __name__ == "__main__":
    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    t_start = time.time()
    main(sys.argv[1] if len(sys.argv) > 1 else "damerau")
    print(f"SECONDS {time.time() - t_start:.1f}")
    print("FAILURES", failures)
    sys.exit(1 if failures else 0)
