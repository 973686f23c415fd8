"""The inputs of tests/test_gpu_layouts_multi.py (the multi-query and join roads on every corpus layout) and of tests/test_layout_multi_inputs.py, which checks on
the host that they are what they are meant to be.  No GPU is needed here; everything is deterministic from fixed seeds.

  P    the scanned corpus: byte candidates of 0..70 symbols (70: the tight cutoffs of join_check.CUTOFFS stay tight), every length holding 64 t + r candidates
       with t in {0, 1, 2} and r in 1..63, so that under RF_NO_MIXED_TILES every length ends in a partial tile.  Forced: length 0 has 5 candidates, length 20
       two full tiles, length 33 one full tile + ONE candidate (a tile with one live lane), length 64 two full tiles + 63, lengths 65..70 no full tile.  The
       order is shuffled; the symbols follow a geometric law over a shuffled alphabet of the bytes 48..121, with a few 0x00 and 0xFF: frequency-rank
       renaming is far from the identity.
  Q    eleven queries of 0, 1, 5, 20, 20, 32, 33, 33, 64, 64 and 65 symbols.  Each is planted into P after 0, 0, 1, 1, 2, 2, 3 and 3 random edits
       (join_check.edits), over a not yet planted candidate of the edited row's own length -- the counts do not change -- and so that, with the k-th
       candidate of a length in original order sitting in that length's tile k // 64, every query has a planted row in a tile with padding lanes and one in
       a full tile (tests/test_layout_multi_inputs.py holds this against rf.host_layout).
  QC   the query corpus of the joins: Q's rows plus filler rows, 70 of 20 symbols, 65 of 33 and three each of 5, 32 and 64 (Q's own counted), one each of 0, 1
       and 65.  The default layout gives it one exact tile per big length and a mixed section, RF_NO_MIXED_TILES partial tiles; Q's first 20-symbol row is the
       first of its length (the full tile), the second the last (the partial tile), and Q's second 33-symbol row is the 65th of its length: the one live lane.
       Three in four filler rows are cut from P, so that the joins match in many tiles: candidates of the same length with up to two substitutions,
       candidates out of the partial tile of the length three symbols longer with three symbols deleted -- a match in the LAST tile of the row's window
       under distance <= 3 -- and candidates out of the first tile of the length three symbols shorter with three symbols inserted: the window's FIRST.

The expectations are the CPU oracle's, through join_check.Oracle (u32; with its rule for the Levenshtein similarity quirk Q2) and join_f64_check.Oracle (f64, every
double by its bit pattern), built once per (corpus, metric, op, cutoff)."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import join_check as J  # noqa: E402
import join_f64_check as F  # noqa: E402
from rapidfuzz_rs_amd import _native as N  # noqa: E402

DIST, SIM, ND, NS = N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
NONE32 = 0xFFFFFFFF
MAX_LEN = 70
QUERY_LENGTHS = [0, 1, 5, 20, 20, 32, 33, 33, 64, 64, 65]
PLANT_EDITS = (0, 0, 1, 1, 2, 2, 3, 3)
FORCED = {0: (0, 5), 20: (2, None), 33: (1, 1), 64: (2, 63), 65: (0, None), 66: (0, None), 67: (0, None), 68: (0, None), 69: (0, None), 70: (0, None)}  # length -> (t, r)
QC_COUNTS = {0: 1, 1: 1, 5: 3, 20: 70, 32: 3, 33: 65, 64: 3, 65: 1}

# what the GPU test runs (tests/test_layout_multi_inputs.py checks the oracle's answers to every one of them)
U32_FILTER = [(metric, op, cutoff) for metric in ("levenshtein", "indel", "lcs_seq") for op in (DIST, SIM) for cutoff in J.CUTOFFS[(metric, op)]]
U32_PER_QUERY = [("levenshtein", DIST, 60), ("osa", DIST, 3)]  # a loose cutoff (plan() sets no early-out); a metric without a fused kernel
F64_FILTER = [("levenshtein", NS, 0.9), ("levenshtein", ND, 0.1), ("indel", NS, 0.9), ("indel", ND, 0.1), ("ratio", SIM, 0.9)]
F64_PER_QUERY = [("jaro_winkler", SIM, 0.9)]
U32_TOPK = [("levenshtein", DIST, None), ("levenshtein", DIST, 40), ("indel", SIM, None)]
F64_TOPK = [("levenshtein", NS, None), ("ratio", SIM, None)]
U32_JOIN = [("levenshtein", DIST, 3), ("indel", DIST, 6)] + [("lcs_seq", SIM, c) for c in J.CUTOFFS[("lcs_seq", SIM)]]
F64_JOIN = [("levenshtein", NS, 0.9), ("indel", ND, 0.1), ("ratio", SIM, 0.9)]


def _symbols(rng, alphabet, size):
    return alphabet[np.minimum(rng.geometric(0.07, size=size) - 1, len(alphabet) - 1)]


def ragged(rows):
    offsets = np.zeros(len(rows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
    data = np.frombuffer(b"".join(rows), dtype=np.uint8).copy()
    return data, offsets


def ranks(rows):
    """rank[i] = how many rows before row i have its length: where a packer that keeps a length's candidates in original order puts it"""
    seen, out = {}, []
    for r in rows:
        out.append(seen.get(len(r), 0))
        seen[len(r)] = out[-1] + 1
    return out


def in_padded_tile(rank, count):
    """under RF_NO_MIXED_TILES: the last tile of a length holds padding lanes (every count here is 64 t + r with r >= 1)"""
    return rank >= 64 * (count // 64)


@functools.lru_cache(maxsize=None)
def queries():
    rng = np.random.default_rng(20261101)
    qs = [bytearray(rng.integers(48, 122, size=ln, dtype=np.uint8).tobytes()) for ln in QUERY_LENGTHS]
    qs[3][7], qs[6][11], qs[8][40] = 0xFF, 0x00, 0xFF  # (bytes whose frequency rank differs most from their value)
    qs = [bytes(q) for q in qs]
    assert len(set(qs)) == len(qs) and not any(b"~" in q for q in qs)
    return qs


@functools.lru_cache(maxsize=None)
def scanned():
    """P: cands, data, offsets, counts {length: candidates}, planted {query: [(edits, candidate index)]}, rank (of every candidate within its length)"""
    rng = np.random.default_rng(20261102)
    counts = {}
    for ln in range(MAX_LEN + 1):
        t, r = int(rng.integers(0, 3)), int(rng.integers(1, 64))
        ft, fr = FORCED.get(ln, (None, None))
        counts[ln] = 64 * (t if ft is None else ft) + (r if fr is None else fr)
    per = np.repeat(np.arange(MAX_LEN + 1), [counts[ln] for ln in range(MAX_LEN + 1)])
    rng.shuffle(per)
    alphabet = rng.permutation(np.arange(48, 122, dtype=np.uint8))
    cands = [bytearray(_symbols(rng, alphabet, int(ln)).tobytes()) for ln in per]
    for i in rng.choice(len(cands), size=40, replace=False):  # a few 0x00 and 0xFF
        if cands[i]:
            cands[i][int(rng.integers(0, len(cands[i])))] = 0x00 if i % 2 else 0xFF
    cands = [bytes(c) for c in cands]
    rank = ranks(cands)
    free = {}  # length -> {padded?: [candidate indices not yet planted]}
    for i, c in enumerate(cands):
        free.setdefault(len(c), {True: [], False: []})[in_padded_tile(rank[i], counts[len(c)])].append(i)
    planted = {}
    for qi, q in enumerate(queries()):
        # the eight edited rows are drawn again (from the same generator) until their lengths have free candidates in a padded and in a full tile
        for _attempt in range(1000):
            trial = {ln: {k: list(v) for k, v in kinds.items()} for ln, kinds in free.items()}
            rows, ok = [], True
            for j, k in enumerate(PLANT_EDITS):
                row = J.edits(rng, q, k)
                kinds = trial.get(len(row), {True: [], False: []})
                want = j % 2 == 0  # (alternately a padded and a full tile, where the length has both)
                pool = kinds[want] or kinds[not want]
                if not pool:
                    ok = False
                    break
                at = pool.pop(int(rng.integers(0, len(pool))))
                rows.append((k, at, row))
            tiles = {in_padded_tile(rank[at], counts[len(row)]) for _, at, row in rows} if ok else set()
            if tiles == {True, False}:
                break
        else:
            raise AssertionError(f"query {qi}: no planting with a padded and a full tile")
        free = trial
        for _, at, row in rows:
            cands[at] = row
        planted[qi] = [(k, at) for k, at, _ in rows]
    data, offsets = ragged(cands)
    return SimpleNamespace(cands=cands, data=data, offsets=offsets, counts=counts, planted=planted, rank=rank, n=len(cands))


@functools.lru_cache(maxsize=None)
def query_corpus():
    """QC: rows, data, offsets, counts, qrow (row index of every query of Q), rank, padded (rows in a tile with padding lanes under RF_NO_MIXED_TILES)"""
    rng = np.random.default_rng(20261103)
    p, qs = scanned(), queries()
    alphabet = np.arange(48, 122, dtype=np.uint8)
    by_len = {}
    for i, c in enumerate(p.cands):
        by_len.setdefault(len(c), []).append(i)
    def pick(ln, last_tile):
        """a candidate of P of ln symbols out of the last (partial) or the first tile of its length"""
        pool = [i for i in by_len[ln] if (in_padded_tile(p.rank[i], p.counts[ln]) if last_tile else p.rank[i] < 64)]
        return bytearray(p.cands[pool[int(rng.integers(0, len(pool)))]])

    filler = []
    for ln, count in QC_COUNTS.items():
        for j in range(count - QUERY_LENGTHS.count(ln)):
            kind = j % 4
            if kind == 0:    # three symbols longer in P, in the LAST tile of a distance-3 window: a candidate of the partial tile of ln + 3 with three symbols deleted
                row = pick(ln + 3, True)
                for at in sorted(rng.choice(ln + 3, size=3, replace=False).tolist(), reverse=True):
                    del row[at]
            elif kind == 1:  # a candidate of P of the same length with 0..2 substitutions
                row = pick(ln, j % 8 == 1)
                for at in rng.integers(0, ln, size=j % 3):
                    row[int(at)] = 126
            elif kind == 2:  # three symbols shorter in P, in the FIRST tile of the window: a candidate of the first tile of ln - 3 with three symbols inserted
                row = pick(ln - 3, False)
                for at in rng.integers(0, ln - 2, size=3):
                    row.insert(int(at), 126)
            else:
                row = bytearray(_symbols(rng, alphabet, ln).tobytes())
            assert len(row) == ln
            filler.append(bytes(row))
    filler = [filler[int(i)] for i in rng.permutation(len(filler))]
    head, tail = [0, 1, 2, 3, 5, 6, 8], [4, 7, 9, 10]
    rows = [qs[i] for i in head] + filler + [qs[i] for i in tail]
    qrow = [0] * len(qs)
    for at, i in enumerate(head):
        qrow[i] = at
    for at, i in enumerate(tail):
        qrow[i] = len(head) + len(filler) + at
    counts = {ln: sum(1 for r in rows if len(r) == ln) for ln in sorted({len(r) for r in rows})}
    rank = ranks(rows)
    padded = [i for i, r in enumerate(rows) if in_padded_tile(rank[i], counts[len(r)])]
    data, offsets = ragged(rows)
    return SimpleNamespace(rows=rows, data=data, offsets=offsets, counts=counts, qrow=qrow, rank=rank, padded=padded, n=len(rows))


def join_query_indices():
    """the rows of QC in padded tiles plus the 65-symbol row, unordered and with repeats"""
    qc = query_corpus()
    rng = np.random.default_rng(20261104)
    rows = sorted(set(qc.padded) | {qc.qrow[10]})
    qi = rows + [rows[int(i)] for i in rng.integers(0, len(rows), size=6)]
    return [qi[int(i)] for i in rng.permutation(len(qi))]


def pad_map(counts):
    """the slot map's padding under RF_NO_MIXED_TILES, as test_gpu_layouts._check_layout computes it: one run of ceil(count / 64) tiles per length, ascending,
    padding at the end of its last tile.  Returns (pad bool[slots], tile_len int[tiles])."""
    pad, tile_len = [], []
    for ln in sorted(counts):
        t = -(-counts[ln] // 64)
        pad += [False] * counts[ln] + [True] * (64 * t - counts[ln])
        tile_len += [ln] * t
    return np.array(pad, dtype=bool), np.array(tile_len, dtype=np.int64)


def window(tile_len, len1, cutoff):
    """[tile_begin, tile_end) of plan() for Levenshtein distance <= cutoff: from the first tile of the first run of the length table (the runs of equal tile
    length, in tile order) whose length is within the cutoff of len1 to the end of the last such run; (0, 0) when there is none"""
    hit = np.nonzero(np.abs(np.asarray(tile_len, dtype=np.int64) - len1) <= cutoff)[0]
    if not len(hit):
        return 0, 0
    tl = list(tile_len)
    b, e = int(hit[0]), int(hit[-1]) + 1
    while b > 0 and tl[b - 1] == tl[b]:
        b -= 1
    while e < len(tl) and tl[e] == tl[e - 1]:
        e += 1
    return b, e


def _corpus(which):
    c = {"P": scanned, "QC": query_corpus}[which]()
    return c.data, c.offsets


@functools.lru_cache(maxsize=None)
def oracle_u32(which, metric, op, cutoff):
    return J.Oracle(metric, op, cutoff, *_corpus(which))


@functools.lru_cache(maxsize=None)
def oracle_f64(which, metric, op, cutoff):
    return F.Oracle(metric, op, cutoff, *_corpus(which))


def descending(op):
    return op in (SIM, NS)


@functools.lru_cache(maxsize=None)
def somes(is_f, metric, op, cutoff, q):
    """(indices int64[m], scores[m]) of the oracle's Somes of query q over P, ascending index; f64 scores as doubles"""
    if is_f:
        idx, bits = oracle_f64("P", metric, op, cutoff).row(q)
        return np.array(idx, dtype=np.int64), np.array(bits, dtype=np.uint64).view(np.float64)
    idx, sc = oracle_u32("P", metric, op, cutoff).row(q)
    return idx.astype(np.int64), sc


def ranked(is_f, metric, op, cutoff, q):
    """the Somes by (score, index), best first"""
    idx, sc = somes(is_f, metric, op, cutoff, q)
    v = sc.astype(np.float64)  # (u32 scores are exact in a double)
    order = np.lexsort((idx, -v if descending(op) else v))
    return idx[order], sc[order]


def bits(s):
    return np.ascontiguousarray(s, dtype=np.float64).view(np.uint64).tolist()


def score_list(is_f, s):
    """scores as comparable Python values: u32 as ints, f64 as 64-bit patterns"""
    return bits(s) if is_f else np.asarray(s).astype(np.uint32).tolist()
