"""The general top-k path (rf_api_topk.hip select_topk over rf_select.hip), topk_scores_kernel and the device merges on keys that the scores of random
short strings never produce: u32 keys that need three radix digits, descending u32 keys with their high bits set, tie classes that end at, just behind and
inside a block of 2048 scores, more than 2048 x 256 scores, corpora with no or a few valid scores, score vectors that start 4, 8 and 12 bytes into an
allocation, and merges of synthetic keys and entries.

Scores come from the CPU oracle and a selection is numpy.lexsort of the full oracle result (tests/topk_select_check.py has the references, the corpora
and the checker of the result roads).  What a corpus is there for is asserted from the oracle's values before the device is called: a corpus that does not
reach the branch fails its test."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd import parallel
from rapidfuzz_rs_amd.utils import synth

import topk_select_check as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _none(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad[:8])


def _child(mode, **env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "topk_select_check.py"), mode], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, **env), timeout=600)
    assert r.returncode == 0 and "FAILURES 0" in r.stdout.splitlines()[-1:], r.stdout[-3000:] + r.stderr[-3000:]
    return r


# ---------------------------------------------------------------------------------------------------------------- 1. three digit passes, ascending
N_RAGGED = 20_011
W_GENERAL = (65535, 65521, 65497)


@functools.lru_cache(maxsize=None)
def _case1():
    q, data, offsets, at = T.planted_ragged(N_RAGGED, 40, 101)
    full = T.oracle_full("levenshtein", q, N.OP_DISTANCE, data, offsets, weights=W_GENERAL)
    return q, rf.Corpus.from_ragged(data, offsets), full, at


@pytest.mark.parametrize("k", [65, 300, 5000, N_RAGGED, N_RAGGED + 7])
def test_u32_keys_over_three_digit_passes(k):
    """Levenshtein distance under the weights (65535, 65521, 65497): the distances span 0 .. ~6.2 M, so select_topk starts at bit 22 and walks three
    digits (bits 22..12, 11..1 and a last digit of ONE bit), carrying `prefix` / `prefix_mask` from pass to pass -- every other u32 score of the suite is
    below 2048 and ends after one pass with shift 0"""
    q, corpus, full, at = _case1()
    assert (full != T.U64MAX).all()
    lo, hi = int(full.min()), int(full.max())
    assert lo == 0 and T.highest_bit(lo ^ hi) >= 22, (lo, hi)  # (condition) three passes of 11 bits at most
    assert len(np.unique(full)) >= 1000  # (condition) the digits below the first one matter
    assert 40 <= int((full[at] == 0).sum()) <= 60 and len(at) >= 240
    bc = rf.distance.levenshtein.BatchComparator(q)
    _none(T.check_roads("weights (65535, 65521, 65497)", bc, corpus, N.OP_DISTANCE, k, full, False, {"weights": W_GENERAL}))


# ---------------------------------------------------------------------------------------------------------------- 2. descending u32 keys
W_UNIFORM = (60000, 60000, 60000)


@functools.lru_cache(maxsize=None)
def _case2():
    q, data, offsets, at = T.planted_ragged(N_RAGGED, 80, 202)
    sim = T.oracle_full("levenshtein", q, N.OP_SIMILARITY, data, offsets, weights=W_UNIFORM)
    cutoff = int(np.median(sim)) + 1
    return q, rf.Corpus.from_ragged(data, offsets), sim, cutoff, T.oracle_full_q2(q, data, offsets, cutoff, weights=W_UNIFORM)


@pytest.mark.parametrize("cut", [False, True], ids=["uncut", "cutoff"])
@pytest.mark.parametrize("k", [65, 1000, N_RAGGED])
def test_u32_keys_descending_with_high_bits_set(k, cut):
    """Levenshtein similarity under the weights (60000, 60000, 60000): similarities 0 .. 4.8 M, so the descending keys 0xFFFFFFFE - s have bits 31..23 set
    and differ from bit 22 down: the `prefix_mask &= 0xFFFFFFFF` line trims a mask that reaches beyond the key, and the first digit sits on top of a
    prefix of ones.  With k = n the similarities of 0 come last and are not dropped; under a cutoff half of the candidates are None."""
    q, corpus, sim, cutoff, sim_cut = _case2()
    assert (sim != T.U64MAX).all()
    assert int(sim.max()) >= 2**22 and int(sim.min()) == 0  # (conditions) a similarity beyond 2^22, similarities of 0
    full = sim_cut if cut else sim
    keys = 0xFFFFFFFE - full[full != T.U64MAX].astype(np.int64)
    assert T.highest_bit(int(keys.min()) ^ int(keys.max())) >= 22  # (condition) more than one pass, below a prefix of set bits
    kw = {"weights": W_UNIFORM}
    if cut:
        kw["score_cutoff"] = cutoff
        assert 3 * int((full == T.U64MAX).sum()) >= N_RAGGED and int((full != T.U64MAX).sum()) > 1000  # (condition) a third or more are None
    elif k == N_RAGGED:
        ev, ei = T.select(full, k, True, False)
        assert len(ev) == N_RAGGED and int(ev[-1]) == 0  # the zeros are the tail of the expected list
    bc = rf.distance.levenshtein.BatchComparator(q)
    _none(T.check_roads(f"weights (60000, 60000, 60000) similarity {kw.get('score_cutoff')}", bc, corpus, N.OP_SIMILARITY, k, full, False, kw))


# ---------------------------------------------------------------------------------------------------------------- 3. tie classes and block boundaries
N_TIES = 3 * 2048 + 77
TIE_SCORERS = {"levenshtein-distance": ("levenshtein", N.OP_DISTANCE, 65), "levenshtein-normalized_similarity": ("levenshtein", N.OP_NORMALIZED_SIMILARITY, 1),
               "jaro_winkler-similarity": ("jaro_winkler", N.OP_SIMILARITY, 1)}


@functools.lru_cache(maxsize=None)
def _case3(name):
    metric, op, min_k = TIE_SCORERS[name]
    q, rows, data, offsets = T.fixed_length(N_TIES, 12, b"ab", 303)
    full = T.oracle_full(metric, q, op, data, offsets)
    return q, rf.Corpus.from_rows(rows), full, T.tie_ks(full, T.descending(op), T.is_float(metric, op), min_k)


@pytest.mark.parametrize("place", ["a", "b", "c", "d"])
@pytest.mark.parametrize("name", list(TIE_SCORERS))
def test_tie_classes_against_block_boundaries(name, place):
    """3 x 2048 + 77 candidates of 12 symbols over "ab": a dozen distances.  k from the oracle's cumulative counts: (a) the end of a tie class, (b) one
    past it (need_eq = 1), (c) inside a class with the quota used up among the first 2048 indices (the later blocks' equal keys must stay out), (d) inside
    a class with the quota used up in the last, partial block (tests/topk_select_check.py tie_ks asserts that the scores have these places)"""
    metric, op, min_k = TIE_SCORERS[name]
    q, corpus, full, ks = _case3(name)
    if metric == "levenshtein" and op == N.OP_DISTANCE:
        assert 6 <= len(np.unique(full)) <= 13
    bc = getattr(rf.distance, metric).BatchComparator(q)
    _none(T.check_roads(f"ties {name} ({place})", bc, corpus, op, ks[place], full, T.is_float(metric, op), {}))


# ---------------------------------------------------------------------------------------------------------------- 4. beyond 2048 x 256 scores
def test_more_than_2048_x_256_scores():
    """2048 x 257 + 5 candidates: sel_scan_kernel's 256 threads own two blocks of counts each (`per` = 2; the last thread that has any owns one), which no
    corpus compared with a reference reached"""
    _none(T.large_failures())


def test_more_than_2048_x_256_scores_one_workgroup_per_cu():
    """the same in a child process with RF_SCAN_BLOCKS_PER_CU=1: the grid-stride loops of sel_minmax_kernel and sel_hist_kernel take several trips"""
    _child("large", RF_SCAN_BLOCKS_PER_CU="1")


# ---------------------------------------------------------------------------------------------------------------- 5. few or no valid scores
def _cases_of_few():
    q, rows, data, offsets = T.fixed_length(N_TIES, 12, b"ab", 303)
    yield "nobody", b"c" * 12, rf.Corpus.from_rows(rows), data, offsets, 0, [("levenshtein", N.OP_DISTANCE, 3), ("levenshtein", N.OP_NORMALIZED_SIMILARITY, 0.9),
                                                                              ("jaro_winkler", N.OP_SIMILARITY, 0.9)]
    q = synth.query(40, 505)
    data, offsets = synth.ragged_host(5000, 64, seed=506)
    cands = [data[int(offsets[i]): int(offsets[i + 1])].tobytes() for i in range(5000)]
    for edits, r in enumerate((100, 2500, 4999)):  # one per block of 2048 scores
        b = bytearray(q)
        for pos in range(edits):
            b[7 * pos + 3] = 126
        cands[r] = bytes(b)
    data, offsets = rf.ragged(cands)
    yield "three", q, rf.Corpus.from_ragged(data, offsets), data, offsets, 3, [("levenshtein", N.OP_DISTANCE, 3), ("levenshtein", N.OP_NORMALIZED_DISTANCE, 0.06),
                                                                             ("jaro_winkler", N.OP_SIMILARITY, 0.93)]
    data, offsets = rf.ragged([b"sitting"])
    yield "one", b"kitten", rf.Corpus.from_list([b"sitting"]), data, offsets, 1, [("levenshtein", N.OP_DISTANCE, None), ("levenshtein", N.OP_SIMILARITY, None),
                                                                                ("levenshtein", N.OP_NORMALIZED_SIMILARITY, None), ("jaro_winkler", N.OP_SIMILARITY, None)]


def test_few_or_no_valid_scores():
    """a cutoff nobody passes (count 0, every entry empty), exactly 3 candidates within the cutoff, and a corpus of one candidate: k = 65 and k = 1"""
    bad = []
    for tag, q, corpus, data, offsets, valid, calls in _cases_of_few():
        for metric, op, cutoff in calls:
            kw = {} if cutoff is None else {"score_cutoff": cutoff}
            is_f = T.is_float(metric, op)
            full = T.oracle_full(metric, q, op, data, offsets, **kw)
            assert int(T.valid_of(full, is_f).sum()) == valid, (tag, metric, op)  # (condition)
            for k in (65, 1):
                bad += T.check_roads(f"{tag} {metric} op {op} cutoff {cutoff}", getattr(rf.distance, metric).BatchComparator(q), corpus, op, k, full, is_f, kw)
    _none(bad)


# ---------------------------------------------------------------------------------------------------------------- 6. topk_scores_kernel
def test_topk_scores_kernel_tails_and_unaligned_score_vectors():
    """a 100-symbol Levenshtein query (two words: scan into a score vector + topk_scores_kernel by default) over 64 x 40 + 1..4 candidates whose best match is
    the last one, with `out` absent, on the host, an aligned device tensor, and views 4, 8 and 12 bytes into a device tensor: the kernel's scalar loads,
    for the 1..3 scores behind the last 16-byte vector and for a whole unaligned vector; the sentinels around the views must survive"""
    _none(T.tail_failures("levenshtein", 100))


def test_topk_scores_kernel_forced_for_single_word_levenshtein_and_osa():
    _child("via_scores", RF_TOPK_VIA_SCORES="2")


# ---------------------------------------------------------------------------------------------------------------- 7. merges on synthetic keys
@pytest.mark.parametrize("n", T.KEY_NS)
def test_merge_keys_device_on_synthetic_keys(n):
    """rf_topk_merge_keys_device (topk_final_kernel) on distinct random 64-bit keys, half of them with bit 63 set, a third of them empty, and on an all-empty
    input: sorted(non-empty)[:k], padded with the empty key"""
    import torch

    for seed, all_empty in ((n, False), (n + 1, False), (n + 2, True)):
        keys = T.synthetic_keys(n, 7000 + seed, all_empty)
        if not all_empty and n >= 15:
            some = keys[keys != T.U64MAX]
            assert 0 < len(some) < n and 0 < int((some >> np.uint64(63)).sum()) < len(some)
        dev = torch.from_numpy(keys.view(np.int64)).cuda()
        for k in T.KEY_KS:
            out = torch.full((k + 2,), T.SENTINEL64, dtype=torch.int64, device="cuda")
            parallel.merge_keys_device(dev, k, out)
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint64).tolist()
            assert got[:k] == T.expected_keys(keys, k) and got[k:] == [T.SENTINEL64] * 2, (n, k, all_empty)


@pytest.mark.parametrize("n", T.ENTRY_NS)
def test_merge_entries_device_on_synthetic_entries(n):
    """rf_topk_merge_entries_device (merge_entries_kernel) on entries that share keys and differ in indices on both sides of 2^32, with empties in between,
    for k below, at and beyond n: the tail behind the valid entries has three kinds of writers (threads beyond n, threads beyond the valid count, ranked
    entries), over 1..20 workgroups"""
    import torch

    for seed in (n, n + 1):
        e = T.synthetic_entries(n, 9000 + seed)
        some = [(int(a), int(b)) for a, b in e if not (int(a) == T.EMPTY and int(b) == T.EMPTY)]
        if n >= 255:
            assert 0 < len(some) < n and len(set(some)) == len(some) and len({a for a, _ in some}) <= 9
            assert any(b < 2**32 for _, b in some) and any(b >= 2**32 for _, b in some)
        dev = torch.from_numpy(e.view(np.int64)).cuda()
        for k in T.entry_ks(n):
            out = torch.full((k + 2, 2), T.SENTINEL64, dtype=torch.int64, device="cuda")
            parallel.merge_entries_device(dev, k, out)
            torch.cuda.synchronize()
            got = [tuple(r) for r in out.cpu().numpy().view(np.uint64).tolist()]
            want = T.expected_entries(e, k)
            assert got[k:] == [(T.SENTINEL64, T.SENTINEL64)] * 2, (n, k)
            assert got[:k] == want, (n, k, next((j, got[j], want[j]) for j in range(k) if got[j] != want[j]))
