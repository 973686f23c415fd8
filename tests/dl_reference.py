"""Test-side restatement of rapidfuzz::distance::damerau_levenshtein (the oracle does not know this metric).  A helper, not a test file.

  dl_many(query, rows, lens)     (a) the unrestricted Damerau-Levenshtein distance of one query against n candidates, numpy-vectorised ACROSS
                                     the candidates (the loops run over the two positions only), in linear space
  ops(op, query, rows, lens, cutoff)  (b) the four BatchComparator methods with and without score_cutoff, written from the MetricUsize defaults
                                     (details/distance.rs:154-275) around damerau_levenshtein.rs:170-215 and `score()` (common.rs);
                                     None is 0xFFFFFFFF (u32 ops) / NaN (f64 ops)
  dl_pair(a, b)                  (c) an independent per-pair Lowrance-Wagner full-matrix implementation that holds (a)
"""
import math

import numpy as np

NONE_U32 = 0xFFFFFFFF
OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY = range(4)


def dl_pair(a, b) -> int:
    """(c) Lowrance-Wagner: H[i+1][j+1] = distance of a[:i] and b[:j]; the last row a symbol was seen in and, per row, the last column that matched."""
    n, m = len(a), len(b)
    inf = n + m
    H = [[0] * (m + 2) for _ in range(n + 2)]
    H[0][0] = inf
    for i in range(n + 1):
        H[i + 1][0], H[i + 1][1] = inf, i
    for j in range(m + 1):
        H[0][j + 1], H[1][j + 1] = inf, j
    last_row = {}
    for i in range(1, n + 1):
        last_col = 0
        for j in range(1, m + 1):
            k, l = last_row.get(b[j - 1], 0), last_col
            cost = 1
            if a[i - 1] == b[j - 1]:
                cost, last_col = 0, j
            H[i + 1][j + 1] = min(H[i][j] + cost, H[i + 1][j] + 1, H[i][j + 1] + 1, H[k][l] + (i - k - 1) + 1 + (j - l - 1))
        last_row[a[i - 1]] = i
    return H[n + 1][m + 1]


def pad_rows(cands, dtype=np.int64):
    """list of sequences -> (rows [n, max_len] padded with -1, lens [n])"""
    lens = np.array([len(c) for c in cands], dtype=np.int64)
    rows = np.full((len(cands), int(lens.max()) if len(cands) else 0), -1, dtype=dtype)
    for i, c in enumerate(cands):
        rows[i, : len(c)] = np.frombuffer(c, dtype=np.uint8) if isinstance(c, (bytes, bytearray)) else np.asarray(c, dtype=dtype)
    return rows, lens


def ragged_rows(data, offsets):
    """the (data, offsets) form the corpus packers take -> (rows, lens)"""
    offsets = np.asarray(offsets, dtype=np.int64)
    lens = np.diff(offsets)
    n, width = len(lens), int(lens.max()) if len(lens) else 0
    rows = np.full((n, width), -1, dtype=np.int64)
    col = np.arange(width)[None, :]
    mask = col < lens[:, None]
    rows[mask] = np.asarray(data, dtype=np.int64)[(offsets[:-1, None] + col)[mask]]
    return rows, lens


def dl_many(query, rows, lens) -> np.ndarray:
    """(a) Columns x = 1 .. are the candidates' symbols, the state is a row over the query positions y (Zhao & Sahni's linear-space form of the
    recurrence): besides the previous row R and the one before it R2, per query position the last column K[y] that held the symbol q_y and the
    entry FR[y] = H[K[y]-1][y-2] noted there; per column the last query position Lh that matched and T = H[x-2][Lh-1].  The two transposition
    terms that can win are FR[y] + (x - K[y]) when q_{y-1} matched this column, and T + (y - Lh) when the previous column held q_y."""
    q = np.frombuffer(query, dtype=np.uint8).astype(np.int64) if isinstance(query, (bytes, bytearray)) else np.asarray(query, dtype=np.int64)
    rows = np.asarray(rows)
    lens = np.asarray(lens, dtype=np.int64)
    n, width = rows.shape
    m = len(q)
    inf = m + width + 1
    R = np.repeat(np.arange(m + 1, dtype=np.int64)[:, None], n, axis=1)
    R2 = np.full((m + 1, n), inf, dtype=np.int64)
    FR = np.full((m + 1, n), inf, dtype=np.int64)
    K = np.zeros((m + 1, n), dtype=np.int64)
    res = np.where(lens == 0, m, -1).astype(np.int64)
    for x in range(1, int(lens.max()) + 1 if n else 1):
        ch = rows[:, x - 1]
        new = np.empty_like(R)
        new[0] = x
        T = np.full(n, inf, dtype=np.int64)
        Lh = np.zeros(n, dtype=np.int64)
        for y in range(1, m + 1):
            hit = ch == q[y - 1]
            v = np.minimum(np.minimum(R[y - 1], new[y - 1]), R[y]) + 1
            v = np.where((Lh == y - 1) & (Lh > 0), np.minimum(v, FR[y] + (x - K[y])), v)
            v = np.where((K[y] == x - 1) & (K[y] > 0), np.minimum(v, T + (y - Lh)), v)
            new[y] = np.where(hit, R[y - 1], v)
            FR[y] = np.where(hit, R[y - 2] if y >= 2 else inf, FR[y])
            K[y] = np.where(hit, x, K[y])
            T = np.where(hit, R2[y - 1], T)
            Lh = np.where(hit, y, Lh)
        R2, R = R, new
        res = np.where(lens == x, R[m], res)
    assert (res >= 0).all()
    return res


def _distance(d, len1, len2, cutoff):
    """damerau_levenshtein.rs:170-189 + :198-214: usize::MAX (None here) when the cutoff is below |len1 - len2|, else the TRUE distance"""
    if cutoff is not None and cutoff < abs(len1 - len2):
        return None
    return d


def op_pair(op, d, len1, len2, cutoff=None):
    """(b) one candidate: the value `<op>_with_args` returns for true distance d, None for Option::None.  The usize ops return ints, the normalized ones floats."""
    maximum = max(len1, len2)  # :194-196
    if op == OP_DISTANCE:  # distance_with_args: _distance, then score(): Some iff <= cutoff
        v = _distance(d, len1, len2, cutoff)
        return None if v is None or (cutoff is not None and v > cutoff) else v
    if op == OP_SIMILARITY:  # details/distance.rs:181-211, then score(): Some iff >= cutoff
        if cutoff is not None and cutoff > maximum:
            sim = maximum
        else:
            v = _distance(d, len1, len2, None if cutoff is None else maximum - cutoff)
            if v is None:
                return None  # `maximum - usize::MAX`: a panic / a wrapped value in the reference, None on the device (the header's Q2)
            sim = maximum - v
        return None if cutoff is not None and sim < cutoff else sim
    # :213-252
    nd_cut = cutoff
    if op == OP_NORMALIZED_SIMILARITY and cutoff is not None:
        nd_cut = min(1.0 - cutoff + 0.00001, 1.0)  # common.rs norm_sim_to_norm_dist
    cutoff_distance = None if nd_cut is None else int(math.ceil(maximum * min(max(nd_cut, 0.0), 1.0)))
    v = _distance(d, len1, len2, cutoff_distance)
    nd = math.inf if v is None else (0.0 if maximum == 0 else v / maximum)
    if op == OP_NORMALIZED_DISTANCE:
        return None if cutoff is not None and nd > cutoff else nd
    ns = 1.0 - nd  # :273
    if math.isinf(nd):
        return None
    return None if cutoff is not None and ns < cutoff else ns


def ops(op, query, rows, lens, cutoff=None, dist=None) -> np.ndarray:
    """(b) over a corpus: uint32 with 0xFFFFFFFF = None for distance / similarity, float64 with NaN = None for the normalized ops"""
    d = dl_many(query, rows, lens) if dist is None else dist
    len1 = len(query)
    vals = [op_pair(op, int(di), len1, int(l2), cutoff) for di, l2 in zip(d, lens)]
    if op in (OP_DISTANCE, OP_SIMILARITY):
        return np.array([NONE_U32 if v is None else v for v in vals], dtype=np.uint32)
    return np.array([np.nan if v is None else v for v in vals], dtype=np.float64)
