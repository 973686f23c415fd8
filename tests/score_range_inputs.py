"""The corpora and oracle results that tests/test_score_range_inputs.py (no GPU) and tests/test_gpu_score_range.py share: u32 scores at and above 2^31.

The device finishes every usize metric in 32-bit arithmetic mod 2^32, and plan() refuses a call only when factor x (len1 + max_len) > 0xFFFFFFFE.  So every
score in [2^31, 0xFFFFFFFE] is a legal result and 0xFFFFFFFF is None.  Weights are capped at 65535, so bit 31 needs strings of 32 769 symbols or more; it is
cheap with a short query over long candidates.

What values are reachable:
  * Uniform weights (f, f, f), f <= 65535.  The distance is f x lev.  It reaches 65535 x 65440 = 0xFF9F0060 with a query of 48 symbols over candidates of up to
    65 488 symbols.  The similarity is f x (Mx - lev) <= f x min(len1, len2) <= f x S / 2, S = len1 + len2: under the refusal rule it cannot reach 2^31, and no
    corpus here tries.
  * Indel-like weights (f, f, s) with s >= 2f.  s <= 65535 forces f <= 32767: the tables (32767, 32767, 65534) and (32767, 32767, 65535).  The distance is
    f x (S - 2 lcs).  It reaches 32767 x (131 075 - 96) = 0xFFCF805D with S = 131 075 (the largest score the device can return at all is 32767 x 131 076 = 0xFFFFFFFC).  The similarity is 2 f lcs:
    it reaches 2^31 only with lcs >= 32 769, that is, with a query of more than 32 768 symbols on long_kernel.
  * General tables are refused from (len1 + max_len) x max(w) >= 2^31 on: their values stay below 2^31, and only that boundary matters.
  * lcs_seq, indel, osa and damerau_levenshtein have the factor 1: out of reach.

All symbols come from synth.ALNUM and every generator is seeded.  Each returns (query bytes, data uint8, offsets uint64[n + 1]) and is made once per process;
scores() is the CPU oracle's result for one (corpus, weights, op, cutoff), also made once and handed out read-only."""
import functools

import numpy as np

import topk_select_check as T
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth

BIT31 = 2**31
TOP = 0xFFFFFFFE  # the largest score a call may promise: plan() refuses factor x (len1 + max_len) beyond it
W_UNIFORM = (65535, 65535, 65535)
W_INDEL_EVEN = (32767, 32767, 65534)
W_INDEL_ODD = (32767, 32767, 65535)
W_GENERAL = (65535, 65521, 65497)
QLEN = 48
UNIFORM_MAX_LEN = 65_488  # 65535 x (48 + 65 488) = 0xFFFF0000; one exact tile of 64 plus 6 leftovers have this length
INDEL_MAX_LEN = 131_027  # 32767 x (48 + 131 027) = 0xFFFF7FFD
LONG_QLEN = 33_000
GENERAL_QLEN = 40
GENERAL_MAX_LEN = 32_768 - GENERAL_QLEN  # (40 + 32 728) x 65535 = 2^31 - 32 768: the last accepted worst case


def factor(weights):
    """the common factor f of a table plan() finishes as f x lev or f x indel"""
    ins, dele, sub = weights
    assert ins == dele and (sub == ins or sub >= 2 * ins), weights
    return ins


def _alnum(rng, length):
    return synth.ALNUM[rng.integers(0, 62, size=int(length))]


def _planted(rng, q, lengths):
    """random candidates of these lengths; every third one of 60 symbols or more carries the query verbatim at a random offset, and a candidate within one symbol
    of the query's length is the query after one deletion (one symbol shorter), one substitution (the same length) or one insertion (one longer): what a cutoff of
    3 x f keeps, far below everything else"""
    qa = np.frombuffer(q, dtype=np.uint8)
    cands, long_ones = [], 0
    for length in lengths:
        b = _alnum(rng, length)
        if abs(length - len(qa)) <= 1:
            b = bytearray(q)
            other = int(synth.ALNUM[(int(np.nonzero(synth.ALNUM == qa[30])[0][0]) + 1) % 62])  # an alphanumeric that differs from q[30]
            if length < len(qa):
                del b[17]
            elif length > len(qa):
                b.insert(30, other)
            else:
                b[30] = other
            b = np.frombuffer(bytes(b), dtype=np.uint8).copy()
        if length >= 60:
            if long_ones % 3 == 0:
                at = int(rng.integers(0, length - len(qa) + 1))
                b[at: at + len(qa)] = qa
            long_ones += 1
        cands.append(b)
    offsets = np.zeros(len(cands) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in cands], dtype=np.uint64)
    data = np.concatenate(cands) if cands else np.zeros(0, dtype=np.uint8)
    data.setflags(write=False)
    offsets.setflags(write=False)
    return data, offsets


def _ragged(seed, max_len, edge_lengths):
    rng = np.random.default_rng(seed)
    q = _alnum(rng, QLEN).tobytes()
    lengths = np.concatenate([np.full(70, max_len), rng.integers(100, max_len + 1, size=120), np.array(edge_lengths)])
    rng.shuffle(lengths)
    return (q,) + _planted(rng, q, [int(x) for x in lengths])


@functools.lru_cache(maxsize=None)
def uniform_ragged():
    """a query of 48 symbols (seed 7) over 201 candidates: 70 of 65 488 symbols (one exact tile and 6 leftovers), 120 of 100..65 488, and the lengths around the
    query's own and around 32 768 -- under (65535, 65535, 65535) about two thirds of the distances are >= 2^31"""
    return _ragged(7, UNIFORM_MAX_LEN, (0, 1, 47, 48, 49, 32_767, 32_768, 32_769, 32_815, 32_816, 32_817))


@functools.lru_cache(maxsize=None)
def uniform_single_length():
    """the same query over 200 candidates of 40 000 symbols each: a single-length corpus; every distance is >= 39 952 x 65535 > 2^31.  A random candidate of that
    length holds the query as a subsequence, so its distance is 39 952 x f whether the query was planted or not; every odd candidate that is not a planted one therefore lacks 1..8 of
    the query's symbols altogether (replaced by one the query does not hold), and its distance is larger by f per query position it cannot match"""
    q = uniform_ragged()[0]
    qa = np.frombuffer(q, dtype=np.uint8)
    rng = np.random.default_rng(7 + 1000)
    data, offsets = _planted(rng, q, [40_000] * 200)
    rows = data.reshape(200, 40_000).copy()
    absent = next(int(x) for x in synth.ALNUM if x not in qa)
    for i in range(1, 200, 2):
        if i % 3 == 0:
            continue  # a planted candidate keeps its copy of the query
        rows[i][np.isin(rows[i], qa[: 1 + i // 2 % 8])] = absent
    data = rows.reshape(-1)
    data.setflags(write=False)
    return q, data, offsets


@functools.lru_cache(maxsize=None)
def indel_like_ragged():
    """a query of 48 symbols (seed 8) over 199 candidates: 70 of 131 027 symbols, 120 of 100..131 027, and lengths around the query's own and on both sides of the
    device packer's limit of 65 535 symbols -- for the tables (32767, 32767, 65534) and (32767, 32767, 65535)"""
    return _ragged(8, INDEL_MAX_LEN, (0, 1, 48, 65_487, 65_488, 65_489, 65_490, 65_535, 65_536))


@functools.lru_cache(maxsize=None)
def long_query():
    """a query of 33 000 symbols (seed 8) over 44 candidates: the query after 0..399 random edits (40 of them, the first one verbatim) and random strings of 33 000,
    20 000, 64 and 0 symbols -- under (32767, 32767, 65534) the similarity 2 f lcs of the near-duplicates is >= 2^31"""
    rng = np.random.default_rng(8)
    q = _alnum(rng, LONG_QLEN).tobytes()
    cands = []
    for j in range(40):
        b = bytearray(q)
        for _ in range(0 if j == 0 else int(rng.integers(0, 400))):
            T.edit(rng, b)
        cands.append(np.frombuffer(bytes(b), dtype=np.uint8))
    cands += [_alnum(rng, length) for length in (LONG_QLEN, 20_000, 64, 0)]
    offsets = np.zeros(len(cands) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(b) for b in cands], dtype=np.uint64)
    data = np.concatenate(cands)
    data.setflags(write=False)
    offsets.setflags(write=False)
    return q, data, offsets


@functools.lru_cache(maxsize=None)
def general_boundary():
    """a query of 40 symbols (seed 9) over 150 candidates of up to 32 768 - 40 symbols, 20 of them of exactly that length: under (65535, 65521, 65497) the worst
    case (len1 + max_len) x max(w) is 2^31 - 32 768, the last one the general table accepts"""
    rng = np.random.default_rng(9)
    q = _alnum(rng, GENERAL_QLEN).tobytes()
    lengths = np.concatenate([np.full(20, GENERAL_MAX_LEN), rng.integers(0, GENERAL_MAX_LEN + 1, size=130)])
    rng.shuffle(lengths)
    return (q,) + _planted(rng, q, [int(x) for x in lengths])


CORPORA = {"uniform_ragged": uniform_ragged, "uniform_single_length": uniform_single_length, "indel_like_ragged": indel_like_ragged, "long_query": long_query,
           "general_boundary": general_boundary}
# (corpus, weights) of the dense, thresholded and top-k legs
SHORT_FAMILIES = (("uniform_ragged", W_UNIFORM), ("uniform_single_length", W_UNIFORM), ("indel_like_ragged", W_INDEL_EVEN), ("indel_like_ragged", W_INDEL_ODD))


def second_query(name, length=20, seed=77):
    """the other queries of the many_multi / filter_multi / topk_multi legs: `length` symbols, the first half of them the head of the corpus' own query"""
    q = CORPORA[name]()[0]
    rng = np.random.default_rng(seed + length)
    return q[: length // 2] + _alnum(rng, length - length // 2).tobytes()


@functools.lru_cache(maxsize=None)
def scores_of(name, q, weights, op, cutoff=None):
    """the CPU oracle's result of query `q` over corpus `name`: uint64 with UINT64_MAX = None, or float64 with NaN = None; read-only.  Levenshtein similarity
    under a cutoff is the uncut similarity kept where it reaches the cutoff (quirk Q2, topk_select_check.oracle_full_q2)."""
    _, data, offsets = CORPORA[name]()
    if cutoff is None:
        full = T.oracle_full("levenshtein", q, op, data, offsets, weights=weights)
    elif op == N.OP_SIMILARITY:
        full = T.oracle_full_q2(q, data, offsets, cutoff, weights=weights)
    else:
        full = T.oracle_full("levenshtein", q, op, data, offsets, weights=weights, score_cutoff=cutoff)
    full.setflags(write=False)
    return full


def scores(name, weights, op, cutoff=None):
    return scores_of(name, CORPORA[name]()[0], weights, op, cutoff)


def median_cutoff(name, weights, op=N.OP_DISTANCE):
    """the median of the uncut scores (of the non-zero ones for a similarity): a cutoff that keeps about half"""
    full = scores(name, weights, op)
    some = full[full > 0] if op == N.OP_SIMILARITY else full
    return int(np.sort(some)[len(some) // 2])


def distance_cutoffs(name, weights):
    f = factor(weights)
    return (median_cutoff(name, weights), BIT31 - 1, BIT31, TOP, 0xFFFFFFFF, 2**32, 2**40, 0, 3 * f)


def similarity_cutoffs(name, weights):
    return (0, 1, median_cutoff(name, weights, N.OP_SIMILARITY), BIT31, 0xFFFFFFFF, 2**32)


NORMALIZED_CUTOFFS = (0.0, 0.05, 0.5, 1.0)
