"""Inputs, references and the road checker shared by tests/test_gpu_topk_selection.py and tests/test_topk_merge_host.py, and, run as a program, the two
runs of tests/test_gpu_topk_selection.py that need a switch the library reads once per process:

  large        with RF_SCAN_BLOCKS_PER_CU=1.  scan_max_grid() is then one workgroup per CU, so over 2048 x 257 + 5 scores the grid-stride loops of
               sel_minmax_kernel and sel_hist_kernel take several trips (asserted: n > 2 x CUs x 256), while sel_scan_kernel's threads own two blocks of
               2048 scores each.  Levenshtein distance, normalized_similarity and jaro_winkler similarity, every result road, against the lexsort of
               the full oracle result.
  via_scores   with RF_TOPK_VIA_SCORES=2.  A single-word Levenshtein query and an OSA query go through topk_scores_kernel (by default only Levenshtein
               queries of 65..256 symbols do), over the same corpora, tails and `out` pointers as the default road in the test.

The last line printed is `FAILURES <count>`; exit status 0 = none.

Scores come from the CPU oracle.  A selection is numpy.lexsort of the full oracle result: None dropped, order (score, index) or (-score, index) for the
similarity ops, the first min(k, #valid) kept.  Where a call also returns every score, that vector is compared first, so a failure names the scan or the
selection."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import rapidfuzz_rs_amd as rf  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402
from rapidfuzz_rs_amd import parallel  # noqa: E402
from rapidfuzz_rs_amd.utils import synth  # noqa: E402
from oracle import oracle as o  # noqa: E402

U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE32 = np.uint32(0xFFFFFFFF)
EMPTY = 0xFFFFFFFFFFFFFFFF
SENTINEL32 = 0x5A5A5A5A
SENTINEL64 = 0x5A5A5A5A5A5A5A5A
BASE = 2**33 + 12345  # index_base of every call: global indices beyond 2^32


def is_float(metric, op):
    return metric in ("jaro", "jaro_winkler") or op >= N.OP_NORMALIZED_DISTANCE


def descending(op):
    return op in (N.OP_SIMILARITY, N.OP_NORMALIZED_SIMILARITY)


def highest_bit(x):
    """index of the highest set bit, -1 for 0"""
    return int(x).bit_length() - 1


# ---------------------------------------------------------------------------------------------------------------- references
def oracle_full(metric, q, op, data, offsets, **kw):
    """every candidate's score from the CPU oracle (uint64 with UINT64_MAX = None, or float64 with NaN = None)"""
    kw = {key: (tuple(v) if key == "weights" else v) for key, v in kw.items()}
    return getattr(o, metric).BatchComparator(q).many(op, data, offsets, nthreads=8, **kw)


def oracle_full_q2(q, data, offsets, cutoff, **kw):
    """Levenshtein similarity under a cutoff: the oracle's uncut similarity, kept where it reaches the cutoff (quirk Q2, tests/test_gpu_parity.py
    _check_many: above the cutoff the reference returns a wrapped sentinel where every in-range entry implies None)"""
    sim = oracle_full("levenshtein", q, N.OP_SIMILARITY, data, offsets, **kw)
    return np.where(sim >= np.uint64(cutoff), sim, U64MAX)


def valid_of(full, is_f):
    return ~np.isnan(full) if is_f else full != U64MAX


def select(full, k, desc, is_f):
    """(scores, indices) of the k best: numpy.lexsort of the full result by (score, index) / (-score, index), None dropped"""
    idx = np.arange(len(full), dtype=np.uint64)
    keep = valid_of(full, is_f)
    v, i = full[keep], idx[keep]
    key = v if is_f else v.astype(np.int64)
    order = np.lexsort((i, -key if desc else key))[:k]
    return v[order], i[order]


def expected_out(full, is_f):
    return full if is_f else np.where(full == U64MAX, NONE32, full.astype(np.uint32))


def same_scores(got, exp, is_f):
    return ((got == exp) | (np.isnan(got) & np.isnan(exp))) if is_f else (got == exp)


# ---------------------------------------------------------------------------------------------------------------- the roads
ROADS = ("topk", "host_out", "device_out", "entries")


def check_roads(tag, bc, corpus, op, k, full, is_f, kw, roads=ROADS):
    """One (scorer, corpus, op, k, args) through every public road -- topk (rf_topk_u32 / rf_topk_f64), topk with a host `out`, with a device `out`, and
    topk_entries_device, decoded with parallel.decode_entries -- against `full`, the oracle's scores.  Returns the failures as strings."""
    import torch

    desc = descending(op)
    n = len(full)
    ev, ei = select(full, k, desc, is_f)
    want = list(zip(ev.tolist(), (ei + np.uint64(BASE)).tolist()))
    exp_out = expected_out(full, is_f)
    bad = []

    def selection(road, pairs):
        if pairs != want:
            at = next((j for j, (g, w) in enumerate(zip(pairs, want)) if g != w), min(len(pairs), len(want)))
            bad.append(f"{tag} k={k} {road}: SELECTION differs: {len(pairs)} entries for {len(want)}, first at {at}: got {pairs[at:at + 2]} want {want[at:at + 2]}")

    def scan(road, got):
        wrong = np.nonzero(~same_scores(got, exp_out, is_f))[0]
        if len(wrong):
            bad.append(f"{tag} k={k} {road}: SCAN differs at {len(wrong)} of {n}, first {wrong[:3].tolist()}: got {got[wrong[:3]].tolist()} want {exp_out[wrong[:3]].tolist()}")

    for road in roads:
        if road == "topk":
            s, i = bc.topk(corpus, k, op, index_base=BASE, **kw)
        elif road == "host_out":
            out = np.full(n, np.nan if is_f else SENTINEL32, dtype=np.float64 if is_f else np.uint32)
            s, i = bc.topk(corpus, k, op, index_base=BASE, out=out, **kw)
            scan(road, out)
        elif road == "device_out":
            out = torch.full((n + 4,), SENTINEL32, dtype=torch.float64 if is_f else torch.int32, device="cuda")
            s, i = bc.topk(corpus, k, op, index_base=BASE, out=out, **kw)
            torch.cuda.synchronize()
            host = out.cpu().numpy()
            scan(road, host[:n] if is_f else host[:n].view(np.uint32))
            if (host[n:] != SENTINEL32).any():
                bad.append(f"{tag} k={k} {road}: wrote behind the {n} scores: {host[n:].tolist()}")
        else:
            ent = torch.full((k + 2, 2), SENTINEL64, dtype=torch.int64, device="cuda")
            bc.topk_entries_device(corpus, k, ent, op, index_base=BASE, **kw)
            torch.cuda.synchronize()
            raw = ent.cpu().numpy()
            if (raw[k:] != SENTINEL64).any():
                bad.append(f"{tag} k={k} {road}: wrote behind the {k} entries")
            if (raw[len(want):k] != -1).any() or (raw[:len(want)] == -1).all(axis=1).any():
                bad.append(f"{tag} k={k} {road}: the empty entries are not exactly the last {k - len(want)}")
            selection(road, parallel.decode_entries(np.ascontiguousarray(raw[:k]), op, is_f))
            continue
        selection(road, list(zip(s.tolist(), i.tolist())))
    return bad


# ---------------------------------------------------------------------------------------------------------------- corpora
def edit(rng, b, alphabet=synth.ALNUM):
    """one random substitution, insertion or deletion, in place"""
    r = int(rng.integers(0, 3))
    pos = int(rng.integers(0, len(b)))
    sym = int(alphabet[int(rng.integers(0, len(alphabet)))])
    if r == 0:
        b[pos] = sym
    elif r == 1:
        b.insert(pos, sym)
    else:
        del b[pos]


@functools.lru_cache(maxsize=None)
def planted_ragged(n, qlen, seed, stride=79):
    """an alphanumeric query of `qlen` symbols against n ragged candidates of 0..100 symbols; every `stride`-th candidate (coprime to 64: every lane of a
    tile gets its turn) is the query, every fifth of them verbatim, the others after 1..3 edits.  Returns (query, data, offsets, planted indices)."""
    rng = np.random.default_rng(seed)
    q = synth.ALNUM[rng.integers(0, 62, size=qlen)].tobytes()
    data, offsets = synth.ragged_host(n, 100, seed=seed + 1)
    cands = [data[int(offsets[i]): int(offsets[i + 1])].tobytes() for i in range(n)]
    at = list(range(5, n, stride))
    for j, r in enumerate(at):
        b = bytearray(q)
        if j % 5:
            for _ in range(1 + j % 3):
                edit(rng, b)
        cands[r] = bytes(b)
    data, offsets = rf.ragged(cands)
    return q, data, offsets, np.array(at)


@functools.lru_cache(maxsize=None)
def fixed_length(n, length, letters, seed):
    """(query, data, offsets) of n candidates of one length over a small alphabet, the query of the same length: a handful of score values, huge tie classes"""
    alphabet = np.frombuffer(letters, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    q = alphabet[rng.integers(0, len(alphabet), size=length)].tobytes()
    rows = alphabet[rng.integers(0, len(alphabet), size=(n, length))]
    return q, rows, rows.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(length)


def tie_ks(full, desc, is_f, min_k, n_blocks_full=3, block=2048):
    """k at the four places of a tie class that the emit pass treats differently, from the oracle's cumulative counts: (a) the end of a class, (b) one past
    it (need_eq = 1), (c) inside a class, the quota running out among the first 2048 indices, (d) inside a class, the quota running out in the last,
    partial block.  Every k >= min_k; asserts that the scores have such places."""
    keep = valid_of(full, is_f)
    assert keep.all()
    key = -full if desc and is_f else (-full.astype(np.int64) if desc else (full if is_f else full.astype(np.int64)))
    values, counts = np.unique(key, return_counts=True)
    cum = np.cumsum(counts)
    j = int(np.searchsorted(cum, min_k))  # the first class that ends at or beyond min_k
    assert j + 1 < len(values), (min_k, cum[:4])
    ks = {"a": int(cum[j]), "b": int(cum[j]) + 1}
    # (c), (d): the largest class among those with min_k scores or more below or inside it
    big = j + int(np.argmax(counts[j:]))
    less = int(cum[big]) - int(counts[big])
    members = np.nonzero(key == values[big])[0]
    first = int((members < block).sum())
    before_last = int((members < n_blocks_full * block).sum())
    assert first >= 2 and before_last > first and len(members) - before_last >= 2, (len(members), first, before_last)
    need_c = max(first // 2, min_k - less, 1)
    assert members[need_c - 1] < block and need_c < len(members), (need_c, first)
    need_d = before_last + (len(members) - before_last + 1) // 2
    assert members[need_d - 1] >= n_blocks_full * block and need_d < len(members), (need_d, before_last, len(members))
    ks["c"], ks["d"] = less + need_c, less + need_d
    assert all(k >= min_k for k in ks.values()), ks
    return ks


# ---------------------------------------------------------------------------------------------------------------- case 4
LARGE_N = 2048 * 257 + 5
LARGE_CALLS = [("levenshtein", N.OP_DISTANCE, (65, 1000)), ("levenshtein", N.OP_NORMALIZED_SIMILARITY, (1, 16, 1000)), ("jaro_winkler", N.OP_SIMILARITY, (300,))]


def large_failures(log=None):
    """beyond 2048 x 256 scores: sel_scan_kernel's threads own two count blocks each (per = ceil(257 / 256) = 2), and n is no multiple of anything"""
    q, rows, data, offsets = fixed_length(LARGE_N, 16, b"abcd", 404)
    assert -(-LARGE_N // 2048) > 256  # per >= 2
    corpus = rf.Corpus.from_rows(rows)
    bad = []
    for metric, op, ks in LARGE_CALLS:
        is_f = is_float(metric, op)
        full = oracle_full(metric, q, op, data, offsets)
        bc = getattr(rf.distance, metric).BatchComparator(q)
        for k in ks:
            got = check_roads(f"large {metric} op {op}", bc, corpus, op, k, full, is_f, {})
            if log:
                log(f"large {metric} op {op} k={k}: {'ok' if not got else got}")
            bad += got
    return bad


# ---------------------------------------------------------------------------------------------------------------- case 6
TAIL_NS = tuple(64 * 40 + t for t in (1, 2, 3, 4))
TAIL_KS = (1, 16, 64)


@functools.lru_cache(maxsize=None)
def tail_corpora(qlen):
    """{shape: (query, candidates)}: 64 x 40 + 4 candidates, of 100 symbols each ("rows") or of 60..140 ("ragged").  The last four are the query after 3,
    2, 1 and 0 substitutions, so whichever of the four sizes a corpus is cut to, its best match is its LAST candidate: one of the 1..3 scores behind the
    last whole 16-byte vector (or the last lane of the last whole one)."""
    rng = np.random.default_rng(600 + qlen)
    q = synth.ALNUM[rng.integers(0, 62, size=qlen)]
    n = TAIL_NS[-1]
    shapes = {}
    for shape, lens in (("rows", np.full(n, 100)), ("ragged", rng.integers(60, 141, size=n))):
        cands = [synth.ALNUM[rng.integers(0, 62, size=int(L))].tobytes() for L in lens]
        for r in range(7, n - 4, 97):  # something to find further up: the query's head with 6..10 foreign symbols in it, the candidate's own length kept
            b = bytearray(cands[r])
            m = min(qlen, len(b))
            b[:m] = q.tobytes()[:m]
            for pos in rng.choice(m, size=6 + r % 5, replace=False):
                b[int(pos)] = 126
            cands[r] = bytes(b)
        for t in range(4):
            b = q.copy()
            b[rng.choice(qlen, size=3 - t, replace=False)] = 126
            if shape == "rows":  # (a single-length corpus keeps its length: foreign symbols behind the query)
                b = np.concatenate([b, np.full(100 - qlen, 125, dtype=np.uint8)])
            cands[n - 4 + t] = b.tobytes()
        shapes[shape] = (q.tobytes(), cands)
    return shapes


def tail_failures(metric, qlen, log=None):
    """topk_scores_kernel over corpora whose size leaves 1, 2, 3 and 0 scores behind the last 16-byte vector, with every kind of `out`: none, a host array,
    an aligned device tensor, and views 4, 8 and 12 bytes into a device tensor (the kernel then loads scalars throughout)"""
    import torch

    bad = []
    for shape, (q, cands) in tail_corpora(qlen).items():
        bc = getattr(rf.distance, metric).BatchComparator(q)
        for n in TAIL_NS:
            data, offsets = rf.ragged(cands[:n])
            full = oracle_full(metric, q, N.OP_DISTANCE, data, offsets)
            # condition: the best match is the last candidate, alone at its score
            assert int(np.argmin(full)) == n - 1 and int((full == full.min()).sum()) == 1, (shape, n)
            exp_out = expected_out(full, False)
            corpus = rf.Corpus.from_ragged(data, offsets) if shape == "ragged" else rf.Corpus.from_rows(np.ascontiguousarray(data, dtype=np.uint8).reshape(n, 100))
            for k in TAIL_KS:
                tag = f"tail {metric} len1={qlen} {shape} n={n}"
                got = check_roads(tag, bc, corpus, N.OP_DISTANCE, k, full, False, {})
                ev, ei = select(full, k, False, False)
                want = list(zip(ev.tolist(), ei.tolist()))
                for j in (1, 2, 3):
                    buf = torch.full((n + 8,), SENTINEL32, dtype=torch.int32, device="cuda")
                    view = buf[j:]
                    assert view.data_ptr() % 16 != 0 and view.data_ptr() % 4 == 0
                    s, i = bc.topk(corpus, k, N.OP_DISTANCE, out=view)
                    torch.cuda.synchronize()
                    host = buf.cpu().numpy().view(np.uint32)
                    if (host[:j] != SENTINEL32).any() or (host[j + n:] != SENTINEL32).any():
                        got.append(f"{tag} k={k} out=buf[{j}:]: a sentinel around the scores is gone: {host[:j].tolist()} {host[j + n:].tolist()}")
                    wrong = np.nonzero(host[j: j + n] != exp_out)[0]
                    if len(wrong):
                        got.append(f"{tag} k={k} out=buf[{j}:]: SCAN differs at {wrong[:4].tolist()}: got {host[j: j + n][wrong[:4]].tolist()} want {exp_out[wrong[:4]].tolist()}")
                    if list(zip(s.tolist(), i.tolist())) != want:
                        got.append(f"{tag} k={k} out=buf[{j}:]: SELECTION differs: got {list(zip(s.tolist(), i.tolist()))[:3]} want {want[:3]}")
                if log:
                    log(f"{tag} k={k}: {'ok' if not got else got}")
                bad += got
    return bad


# ---------------------------------------------------------------------------------------------------------------- case 7: synthetic merge inputs
KEY_NS = (1, 15, 64, 65, 1000, 4099)
KEY_KS = (1, 16, 64)
ENTRY_NS = (1, 255, 256, 257, 5000)


def entry_ks(n):
    return sorted({1, 64, 300, n, n + 9})


def synthetic_keys(n, seed, all_empty=False):
    """n distinct random 64-bit keys, half of them with bit 63 set (as the keys of similarities are), a random third replaced by the empty key"""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < n:
        x = int(rng.integers(0, 2**63 - 1)) | ((len(keys) & 1) << 63)
        if x != EMPTY:
            keys.add(x)
    keys = np.array(sorted(keys), dtype=np.uint64)
    rng.shuffle(keys)
    keys[rng.random(n) < 1 / 3] = U64MAX
    if all_empty:
        keys[:] = U64MAX
    return keys


def expected_keys(keys, k):
    some = sorted(int(x) for x in keys if int(x) != EMPTY)[:k]
    return some + [EMPTY] * (k - len(some))


def synthetic_entries(n, seed):
    """[n, 2] uint64 entries (key, index): keys from a pool of 9 (u32 distances, 0xFFFFFFFF - similarity, f64 images with and without bit 63, and the largest
    key a number can have), so many entries share a key and differ only in the index; indices around 0, just below and just above 2^32 and far beyond it,
    so entries of one key differ only above bit 31 or only below it; (key, index) pairs unique, as rfgpu.h requires; a random third empty, interleaved"""
    rng = np.random.default_rng(seed)
    pool = [0, 3, 0xFFFFFFFF - 7, 0xFFFFFFFF, 0x3FF0000000000000, 0x8000000000000000, 0xBFE0000000000001, 0xC000000000000000, EMPTY - 1]
    bases = [0, 2**32 - 40, 2**32, 2**33 + 5, 2**40, 2**63 + 11]
    pairs = set()
    while len(pairs) < n:
        low = int(rng.integers(0, 256))
        idx = bases[int(rng.integers(0, len(bases)))] + low
        if rng.random() < 0.25:
            idx = low + (int(rng.integers(0, 4)) << 32)  # the same low 32 bits on both sides of 2^32
        pairs.add((pool[int(rng.integers(0, len(pool)))], idx))
    e = np.array(sorted(pairs), dtype=np.uint64)
    rng.shuffle(e)
    e[rng.random(n) < 1 / 3] = U64MAX
    return e


def expected_entries(entries, k):
    """a Python sort by (key, index) of the non-empty entries, padded with (2^64 - 1, 2^64 - 1)"""
    some = sorted((int(a), int(b)) for a, b in entries if not (int(a) == EMPTY and int(b) == EMPTY))[:k]
    return some + [(EMPTY, EMPTY)] * (k - len(some))


# ---------------------------------------------------------------------------------------------------------------- the program
def main(mode):
    import torch

    def log(line):
        print(line, flush=True)

    if mode == "large":
        assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert LARGE_N > 2 * cus * 256, (LARGE_N, cus)  # the minmax and histogram loops take several trips
        log(f"{cus} CUs: {-(-LARGE_N // (cus * 256))} trips of the grid-stride loops over {LARGE_N} scores")
        bad = large_failures(log)
    elif mode == "via_scores":
        assert os.environ.get("RF_TOPK_VIA_SCORES") == "2", "run with RF_TOPK_VIA_SCORES=2"
        bad = tail_failures("levenshtein", 40, log) + tail_failures("osa", 40, log)
    else:
        raise SystemExit(f"unknown mode {mode!r}")
    for b in bad:
        print(b)
    print("FAILURES", len(bad))
    return len(bad)


if __name__ == "__main__":
    sys.exit(1 if main(sys.argv[1]) else 0)
