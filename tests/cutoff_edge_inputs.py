"""Inputs of the f64 cutoff-edge tests: seeded corpora, queries, metric / argument sets and the cutoff grid.  Host only: numpy and the CPU oracle, no GPU import.
tests/test_cutoff_edge_inputs.py holds what is built here to its conditions without a GPU; tests/cutoff_edge_check.py (started by tests/test_gpu_cutoff_edges.py)
runs it through the device.

Every f64-valued result ends in a compare of a double with `score_cutoff`, and the library makes that compare -- or something that has to fall the same way -- in
many places, several of them on the host ("Cutoffs that equal a score").  A round decimal cutoff almost never IS a candidate's score, so it cannot
tell `<=` from `<`, a table entry that is one off, or a planned bound that is one too tight.  The grid here is made of the scores themselves: for one
(metric, arguments, op, query, corpus) the corpus is scored by the oracle WITHOUT a cutoff, at most MOST distinct values are picked by rank -- always the smallest
and the largest, the value nearest each planning threshold on the op's own scale, and where asked the quotients k / maximum -- and each picked v gives the three
cutoffs nextafter(v, -1), v, nextafter(v, 2); FIXED is added.  The EXPECTED vector of a cutoff is the oracle called with that cutoff, never the uncut vector
filtered here: for Jaro and Jaro-Winkler the two differ (the reference's filters and its rewritten cutoff flip float edge cases; flips() counts them).

A triple whose neighbours prev(v) and next(v) give the same number of Somes could not catch a flipped compare; cutoff_grid() drops it (both neighbours inside
[0, 1]; seen only in Jaro-Winkler legs, two triples per leg at the most: tests/test_cutoff_edge_inputs.py has the counts and holds every leg to that).

No LCS-family query (Indel, LCS, fuzz ratio, the Indel-like weight tables) is longer than 64 symbols anywhere here, so quirk Q8 of the reference's banded
multi-word LCS cannot apply and no mismatch is excused.
"""
import math

import numpy as np

from oracle import oracle as o

ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
ABCD = np.frombuffer(b"abcd", dtype=np.uint8)
ALPHABETS = {"abcd": ABCD, "alnum": ALNUM}
QUERY_LENGTHS = (1, 5, 32, 33, 40, 64)
OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY = range(4)
OP_NAMES = ("distance", "similarity", "normalized_distance", "normalized_similarity")
FLAG_RATIO_INDEL_NORMALIZATION = 0x1  # RF_FLAG_RATIO_INDEL_NORMALIZATION
NONE_BITS = np.uint64(0x7FF8000000000000)  # the NaN that stands for None on the device
N_RAGGED = 3037  # 47 tiles and a partial one
N_ROWS = 64 * 40 + 17
MOST = 24
THREADS = 8


def prev(v):
    return float(np.nextafter(v, -1.0))


def next_(v):
    return float(np.nextafter(v, 2.0))


FIXED = (0.0, -0.0, 5e-324, 1.0, next_(1.0), -1.0, math.inf)


# ---------------------------------------------------------------------------------------------- metric / argument sets
class Metric:
    """name: the key of the legs; module: the attribute of rapidfuzz_rs_amd.distance (or "ratio"); ops: every f64 op it has; kw: weights / prefix_weight;
    family: "lev" (RAW_LEV, RAW_OSA, the general weight table), "lcs" (the LCS recurrence), "jaro"; flags: RF_FLAG_* of the device call.
    The oracle's RatioBatchComparator is the reference's (normalized similarity of the inner lcs_seq comparator); with the Indel normalization it is Indel's."""

    def __init__(self, name, module, family, ops, oracle_module=None, flags=0, **kw):
        self.name, self.module, self.family, self.ops, self.flags, self.kw = name, module, family, ops, flags, kw
        self.oracle_module = oracle_module or module

    def oracle(self, q):
        if self.oracle_module == "ratio":
            return o.fuzz.RatioBatchComparator(bytes(q))
        return getattr(o, self.oracle_module).BatchComparator(bytes(q))

    def __repr__(self):
        return self.name


NORM = (OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY)
ALL4 = (OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY)
METRICS = [
    Metric("levenshtein", "levenshtein", "lev", NORM),
    Metric("levenshtein(2,2,2)", "levenshtein", "lev", NORM, weights=(2, 2, 2)),
    Metric("levenshtein(1,1,2)", "levenshtein", "lcs", NORM, weights=(1, 1, 2)),
    Metric("levenshtein(2,2,3)", "levenshtein", "lev", NORM, weights=(2, 2, 3)),
    Metric("osa", "osa", "lev", NORM),
    Metric("indel", "indel", "lcs", NORM),
    Metric("lcs_seq", "lcs_seq", "lcs", NORM),
    Metric("ratio", "ratio", "lcs", (OP_NORMALIZED_SIMILARITY,)),
    Metric("ratio(indel)", "ratio", "lcs", (OP_NORMALIZED_SIMILARITY,), oracle_module="indel", flags=FLAG_RATIO_INDEL_NORMALIZATION),
    Metric("jaro", "jaro", "jaro", ALL4),
    Metric("jaro_winkler(0.0)", "jaro_winkler", "jaro", ALL4, prefix_weight=0.0),
    Metric("jaro_winkler(0.1)", "jaro_winkler", "jaro", ALL4, prefix_weight=0.1),
    Metric("jaro_winkler(0.25)", "jaro_winkler", "jaro", ALL4, prefix_weight=0.25),
    Metric("jaro_winkler(0.3)", "jaro_winkler", "jaro", ALL4, prefix_weight=0.3),  # 4 x 0.3 > 1: no jaro_need early-out
]
BY_NAME = {m.name: m for m in METRICS}
FAMILY = {f: [m for m in METRICS if m.family == f] for f in ("lev", "lcs", "jaro")}


def indel_like(f):
    """the weight table (f, f, 2f): f x Indel, maximum f x (len1 + len2)"""
    return Metric(f"levenshtein({f},{f},{2 * f})", "levenshtein", "lcs", NORM, weights=(f, f, 2 * f))


def is_distance(op):
    return op in (OP_DISTANCE, OP_NORMALIZED_DISTANCE)


# ---------------------------------------------------------------------------------------------- queries and corpora
def query(alphabet, length, seed=0):
    return ALPHABETS[alphabet][np.random.default_rng(9000 + 97 * length + seed).integers(0, len(ALPHABETS[alphabet]), size=length)]


def edited(rng, q, edits, symbols):
    """q after `edits` random insertions / deletions / substitutions"""
    row = list(q)
    for _ in range(edits):
        kind = int(rng.integers(0, 3))
        s = int(symbols[rng.integers(0, len(symbols))])
        if kind == 0 or not row:
            row.insert(int(rng.integers(0, len(row) + 1)), s)
        elif kind == 1:
            del row[int(rng.integers(0, len(row)))]
        else:
            row[int(rng.integers(0, len(row)))] = s
    return np.array(row, dtype=np.uint8)


def ragged(alphabet, qlen, n=N_RAGGED):
    """(data, offsets, query): lengths 0..64 and one in sixty up to 80; every fourth candidate is the query after 0..7 edits"""
    rng = np.random.default_rng(40000 + 1000 * len(ALPHABETS[alphabet]) + qlen)
    symbols = ALPHABETS[alphabet]
    q = query(alphabet, qlen)
    rows = []
    for i in range(n):
        if i % 4 == 0:
            rows.append(edited(rng, q, i // 4 % 8, symbols))
        else:
            ln = int(rng.integers(65, 81)) if i % 60 == 7 else int(rng.integers(0, 65))
            rows.append(symbols[rng.integers(0, len(symbols), size=ln)])
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return np.concatenate(rows).astype(np.uint8), offsets, q


def rows(L, qlen, n=N_ROWS, alphabet="alnum"):
    """(uint8 [n, L], query): a single-length corpus over the 62 symbols of ALNUM (the 6-bit image exists, the fill code 63 is free); every fourth row is the query --
    repeated or cut to L symbols -- with 0..7 substitutions by symbols it does not hold there, rows 1 and 2 of every sixteen shifted by one as well"""
    rng = np.random.default_rng(50000 + 100 * L + qlen)
    symbols = ALPHABETS[alphabet]
    q = query(alphabet, qlen, seed=L)
    out = symbols[rng.integers(0, len(symbols), size=(n, L))]
    base = np.resize(q, L) if qlen else None
    for i in range(0, n, 4) if qlen else ():
        row = base.copy()
        k = i // 4 % 8
        at = rng.choice(L, size=min(k, L), replace=False)
        row[at] = symbols[(np.searchsorted(symbols, row[at]) + 1 + rng.integers(0, len(symbols) - 1, size=len(at))) % len(symbols)]  # another symbol than the one there
        if i // 4 % 16 in (1, 2):
            row = np.roll(row, 1)
        out[i] = row
    return np.ascontiguousarray(out), q


def uniform_offsets(r):
    return np.arange(r.shape[0] + 1, dtype=np.uint64) * np.uint64(r.shape[1])


def chars(n=517):
    """a small `char` corpus: (list of str, query str) over Greek, CJK and one symbol beyond the BMP; every fourth candidate is the query after 0..7 edits.
    The oracle takes bytes: to_bytes() maps the 40 symbols to bytes one to one, which no metric here can tell from the symbols themselves."""
    rng = np.random.default_rng(777)
    symbols = np.array([0x3B1 + i for i in range(24)] + [0x4E00 + 7 * i for i in range(15)] + [0x1F600], dtype=np.uint32)
    q = symbols[rng.integers(0, 40, size=33)]
    out = []
    for i in range(n):
        if i % 4 == 0:
            out.append(_edited_u32(rng, q, i // 4 % 8, symbols))
        else:
            out.append(symbols[rng.integers(0, 40, size=int(rng.integers(0, 65)))])
    return out, q, symbols


def _edited_u32(rng, q, edits, symbols):
    index = {int(s): i for i, s in enumerate(symbols)}
    small = edited(rng, np.array([index[int(s)] for s in q], dtype=np.uint8), edits, np.arange(len(symbols), dtype=np.uint8))
    return symbols[small]


def to_bytes(seq, symbols):
    index = {int(s): i + 48 for i, s in enumerate(symbols)}
    return np.array([index[int(s)] for s in seq], dtype=np.uint8)


def to_str(seq):
    return "".join(chr(int(s)) for s in seq)


def jaro_multiword(n=301):
    """(data, offsets, query): candidates of 60..200 symbols for a query of 100 (jaro_block_kernel); every fourth one is the query after 0..7 edits, every fourth
    of those cut or continued to a length of its own"""
    rng = np.random.default_rng(100200)
    q = query("alnum", 100)
    out = []
    for i in range(n):
        if i % 4 == 0:
            row = edited(rng, q, i // 4 % 8, ALNUM)
            if i // 4 % 4 == 3:
                row = np.resize(row, int(rng.integers(60, 201)))
            out.append(row)
        else:
            out.append(ALNUM[rng.integers(0, 62, size=int(rng.integers(60, 201)))])
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(r) for r in out])
    return np.concatenate(out).astype(np.uint8), offsets, q


# (query length, row length, metric names) whose maximum -- the index range of stream_asm_f64_table -- is 255 and 256 (or the first value beyond it): see maximum()
TABLE_EDGE = [
    (64, 191, ("indel", "ratio(indel)", "levenshtein(1,1,2)")), (64, 192, ("indel", "ratio(indel)", "levenshtein(1,1,2)")),
    (64, 255, ("lcs_seq", "ratio")), (64, 256, ("lcs_seq", "ratio")),
    (32, 19, ("levenshtein(5,5,10)",)), (33, 19, ("levenshtein(5,5,10)",)),
]


def maximum(metric, len1, len2):
    """the `maximum` of the usize metrics' normalization (details/distance.rs: the metric's own maximum(len1, len2))"""
    if metric.family == "jaro":
        return 1
    if metric.oracle_module == "indel" or metric.name == "indel":
        return len1 + len2
    if metric.oracle_module in ("lcs_seq", "ratio"):
        return max(len1, len2)
    if metric.module == "osa":
        return max(len1, len2)
    i, d, s = metric.kw.get("weights", (1, 1, 1))
    m = len1 * d + len2 * i  # levenshtein.rs: min(delete all + insert all, substitute the common part + the length difference)
    if len1 >= len2:
        return min(m, len2 * s + (len1 - len2) * d)
    return min(m, len1 * s + (len2 - len1) * i)


# ---------------------------------------------------------------------------------------------- scoring and the grid
class Scorer:
    """the oracle over one corpus -- ("ragged", data, offsets) or ("rows", array) -- for one metric and query"""

    def __init__(self, metric, q, corpus):
        self.metric, self.q, self.corpus = metric, np.asarray(q, dtype=np.uint8), corpus
        self.batch = metric.oracle(self.q)
        self.n = len(corpus[2]) - 1 if corpus[0] == "ragged" else len(corpus[1])

    def __call__(self, op, cutoff=None):
        """f64 [n], NaN = None"""
        kw = dict(self.metric.kw)
        if cutoff is not None:
            kw["score_cutoff"] = cutoff
        if self.corpus[0] == "ragged":
            return self.batch.many(op, self.corpus[1], self.corpus[2], nthreads=THREADS, **kw)
        return self.batch.rows(op, self.corpus[1], nthreads=THREADS, **kw)


def thresholds(metric, op):
    """the planning thresholds on the op's own scale: the Winkler threshold 0.7 and need = 0.6 (where jaro_need starts) for Jaro / Jaro-Winkler, slack 0.7 and 0.4
    (where plan() switches to the early-out kernels: Levenshtein / OSA and the LCS family) for the usize metrics"""
    marks = (0.7, 0.6) if metric.family == "jaro" else (0.7, 0.4)
    on_scale = (not is_distance(op)) if metric.family == "jaro" else is_distance(op)  # (Jaro's marks are similarities, the usize metrics' are distances)
    return [m if on_scale else 1.0 - m for m in marks]


def must_values(values, marks=(), extra=()):
    """the values every grid holds: the smallest, the largest, the nearest to each mark, every `extra` value that the corpus produces"""
    vals = np.unique(values[~np.isnan(values)])
    if not len(vals):
        return set()
    must = {float(vals[0]), float(vals[-1])}
    for m in marks:
        must.add(float(vals[np.argmin(np.abs(vals - m))]))
    have = set(vals.tolist())
    return must | {float(e) for e in extra if float(e) in have}


def pick(values, marks=(), extra=(), most=MOST):
    """at most `most` of the distinct values by rank: must_values() and, while there is room, values spread evenly by rank"""
    vals = np.unique(values[~np.isnan(values)])
    if not len(vals):
        return []
    must = must_values(values, marks, extra)
    room = max(0, most - len(must))
    rest = [float(v) for v in vals[np.unique(np.linspace(0, len(vals) - 1, num=min(room, len(vals))).round().astype(int))] if float(v) not in must] if room else []
    return sorted(must | set(rest[:room]))


def somes(vec):
    return int(np.count_nonzero(~np.isnan(vec)))


def cutoff_grid(scorer, op, extra=(), most=MOST):
    """(cutoffs, picked, dropped): the triples of the picked values whose neighbours tell a flipped compare apart, then FIXED"""
    picked = pick(scorer(op), thresholds(scorer.metric, op), extra, most)
    cutoffs, kept, dropped = [], [], []
    for v in picked:
        lo, hi = prev(v), next_(v)
        if 0.0 <= lo and hi <= 1.0 and somes(scorer(op, lo)) == somes(scorer(op, hi)):
            dropped.append(v)
            continue
        kept.append(v)
        cutoffs += [lo, v, hi]
    return cutoffs + list(FIXED), kept, dropped


def quotients(metric, op, len1, len2, ks=(2, 3, 4, 5)):
    """k x factor / maximum on the op's scale, with the reference's two f64 operations (details/distance.rs:246-250, :273): where plan_band_filter's K crosses 3"""
    mx = maximum(metric, len1, len2)
    f = metric.kw.get("weights", (1, 1, 1))[0]
    return [k * f / mx if is_distance(op) else 1.0 - k * f / mx for k in ks]


def filtered(full, op, cutoff):
    """the uncut vector under the plain compare: what an `ideal` device would answer -- NOT the expected value (flips() counts where the oracle differs)"""
    keep = full <= cutoff if is_distance(op) else full >= cutoff
    return np.where(keep, full, np.nan)


def same(a, b):
    """bit for bit, as u64 patterns"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64) == np.ascontiguousarray(b, dtype=np.float64).view(np.uint64)


def flips(scorer, op, cutoffs):
    """[(cutoff, candidate)]: where the oracle under the cutoff differs from the filtered uncut value (Some / None or the value itself)"""
    full = scorer(op)
    out = []
    for c in cutoffs:
        got, ideal = scorer(op, c), filtered(full, op, c)
        differ = np.nonzero(~((np.isnan(got) & np.isnan(ideal)) | (got == ideal)))[0]
        out += [(c, int(i)) for i in differ]
    return out


# ---------------------------------------------------------------------------------------------- the legs: which corpora, queries and metrics go together
class Case:
    """one corpus and query: `corpus` is what the oracle scores (bytes), `device` what the library packs -- the same, or ("chars", list of str, query str)"""

    def __init__(self, tag, corpus, q, metrics, most, device=None, len2=None, min_tiles=0):
        self.tag, self.corpus, self.q, self.metrics, self.most, self.device, self.len2 = tag, corpus, np.asarray(q, dtype=np.uint8), metrics, most, device or corpus, len2
        self.min_tiles = min_tiles  # multitile cases: the fewest tiles a launch over this corpus may visit (0: no such condition, every road is run)

    def extra(self, metric, op):
        """the quotients k / maximum: Levenshtein (common factor) and OSA, a 64-symbol query over 64-symbol rows"""
        if self.len2 == 64 and len(self.q) == 64 and metric.family == "lev" and metric.name != "levenshtein(2,2,3)":
            return quotients(metric, op, 64, 64)
        return ()


ROW_SHAPES = ((64, 64), (64, 40), (57, 64), (48, 33), (16, 32))  # (row length, query length)
RAGGED_QUERIES = (0,) + QUERY_LENGTHS
FEW_QUERIES = (5, 40, 64)  # the forced roads: a query per kernel width and the one whose Jaro legs flip
# family-alphabet: the ragged corpora under every query; family-alphabet-few: under FEW_QUERIES; rows-family: ROW_SHAPES; rows-family64: its first two shapes
LEG_NAMES = ("lev-alnum", "lev-abcd", "lcs-alnum", "lcs-abcd", "jaro-alnum", "jaro-abcd", "lev-alnum-few", "lcs-alnum-few", "rows-lev", "rows-lcs", "rows-jaro",
             "rows-lev64", "rows-lcs64", "rows-jaro64", "table-edge", "jaro-multiword", "chars")


def leg_cases(leg):
    """the cases of a leg, built on demand"""
    family, _, what = leg.partition("-")
    alphabet, _, few = what.partition("-")
    if alphabet in ALPHABETS:
        for qlen in FEW_QUERIES if few else RAGGED_QUERIES:
            data, offsets, q = ragged(alphabet, qlen)
            yield Case(f"ragged {alphabet} query {qlen}", ("ragged", data, offsets), q, FAMILY[family], MOST if (alphabet, qlen) == ("alnum", 5) else MOST // 2)
    elif family == "rows":
        shapes = ROW_SHAPES[:2] if what.endswith("64") else ROW_SHAPES + (((16, 5),) if what == "jaro" else ())
        for L, qlen in shapes:
            r, q = rows(L, qlen)
            yield Case(f"rows of {L} query {qlen}", ("rows", r), q, FAMILY[what[:-2] if what.endswith("64") else what], MOST if (L, qlen) == (64, 64) else MOST // 2, len2=L)
    elif leg == "table-edge":
        for qlen, L, names in TABLE_EDGE:
            r, q = rows(L, qlen, n=64 * 12 + 5)
            yield Case(f"rows of {L} query {qlen}", ("rows", r), q, [BY_NAME.get(nm) or indel_like(5) for nm in names], MOST // 2, len2=L)
    elif leg == "jaro-multiword":
        data, offsets, q = jaro_multiword()
        yield Case("candidates of 60..200 query 100", ("ragged", data, offsets), q, FAMILY["jaro"], MOST // 2)
    elif leg == "chars":
        cands, q, symbols = chars()
        parts = [to_bytes(c, symbols) for c in cands]
        offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(x) for x in parts])
        data = np.concatenate(parts).astype(np.uint8)
        metrics = [BY_NAME[nm] for nm in ("levenshtein", "osa", "indel", "jaro", "jaro_winkler(0.1)")]
        yield Case("char corpus query 33", ("ragged", data, offsets), to_bytes(q, symbols), metrics, MOST // 2, device=("chars", [to_str(c) for c in cands], to_str(q)))
    else:
        raise KeyError(leg)


# ---------------------------------------------------------------------------------------------- several tiles per wavefront
WAVES = 4  # kWavesPerBlock
MULTITILE_UNITS = 2  # tiles every wavefront owns at least


def planted_rows(rng, q, L, n):
    """uint8 [n, L] over ALNUM like rows(), vectorized: every fourth row is the query cut to L symbols with 0..7 substitutions by other symbols"""
    out = ALNUM[rng.integers(0, 62, size=(n, L))]
    at = np.arange(0, n, 4)
    k = at // 4 % 8
    hit = np.argsort(rng.random((len(at), L)), axis=1).argsort(axis=1) < k[:, None]  # exactly k positions per row
    base = np.broadcast_to(np.resize(q, L), (len(at), L))
    other = ALNUM[(np.searchsorted(ALNUM, base) + 1 + rng.integers(0, 61, size=base.shape)) % 62]
    out[at] = np.where(hit, other, base)
    return np.ascontiguousarray(out)


def multitile_cases(cus):
    """With RF_SCAN_BLOCKS_PER_CU=1 and RF_SCAN_BLOCKS_PER_CU_FULL=1 a scan launch has at most `cus` workgroups of 4 wavefronts (scan_grid(), scan_grid_full(),
    rf_scan.hip), so a launch over T tiles gives every wavefront T // (4 x cus) tiles at least.  Two corpora sized from the CU count, a 64-symbol query:
    a single-length one of 2 x 4 x cus + 1 tiles (the last one partial), and a ragged one of the lengths 63 and 64 with that many exact tiles EACH, so that a
    length window that keeps one length still leaves every wavefront two tiles.  A thin grid: must_values() and two more."""
    W = WAVES * cus
    tiles = MULTITILE_UNITS * W + 1
    q = query("alnum", 64, seed=4242)
    metrics = [BY_NAME[nm] for nm in ("levenshtein", "indel", "jaro_winkler(0.1)")]
    rng = np.random.default_rng(20261020)
    r = planted_rows(rng, q, 64, 64 * tiles - 27)
    yield Case(f"multitile rows of 64, {tiles} tiles", ("rows", r), q, metrics, 6, len2=None, min_tiles=tiles)
    per_len = {L: planted_rows(rng, q, L, 64 * tiles + 37) for L in (63, 64)}
    lens = rng.permutation(np.concatenate([np.full(len(per_len[L]), L) for L in (63, 64)]))
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = np.empty(int(offsets[-1]), dtype=np.uint8)
    starts = offsets[:-1].astype(np.int64)
    for L in (63, 64):
        at = starts[lens == L]
        data[(at[:, None] + np.arange(L)[None, :]).reshape(-1)] = per_len[L].reshape(-1)
    yield Case(f"multitile lengths 63 + 64, {tiles} exact tiles each", ("ragged", data, offsets), q, metrics, 6, min_tiles=tiles)
