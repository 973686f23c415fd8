"""Test-side restatement of rapidfuzz::distance::{hamming, prefix, postfix} (the oracle does not know these metrics).  A helper, not a test file.

  pair(metric, a, b)                       (a) the raw value of one pair by a plain loop: hamming -> the PADDED distance (mismatches over the common
                                               length + the length difference, hamming.rs:138-161), prefix / postfix -> the common affix' length
  raw_many(metric, query, rows, lens)      (b) the same for one query against n candidates, numpy-vectorised across the candidates
  op_pair(metric, op, raw, len1, len2, cutoff, pad)   (c) what `<op>_with_args` returns: a value, None, or ERR for hamming's Err(DifferentLengthArgs)
                                               (hamming.rs:232-234) -- written from the MetricUsize defaults (details/distance.rs:154-274) around
                                               hamming.rs:165-187 (which overrides _distance) and prefix.rs / postfix.rs:47-69 (which override
                                               _similarity), and `score()` (common.rs:43-45, :83-85)
  ops(metric, op, query, rows, lens, ...)  (c) over a corpus: uint32 with NONE_U32 / DIFFERENT_LENGTH_U32, float64 with the two NaNs
  keep(values)                             what a filter_map over those results keeps: neither None nor Err
score_hint changes nothing in any of the three (hamming.rs:176-187 and the affix scans ignore it), so it is no parameter here.
"""
import math

import numpy as np

from dl_reference import pad_rows, ragged_rows  # noqa: F401  (the same row form: [n, max_len] padded with -1, and the lengths)

NONE_U32 = 0xFFFFFFFF
DIFFERENT_LENGTH_U32 = 0xFFFFFFFE
NONE_F64_BITS = 0x7FF8000000000000
DIFFERENT_LENGTH_F64_BITS = 0x7FF8000000000001
OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY = range(4)
METRICS = ("hamming", "prefix", "postfix")


class _Err:
    def __repr__(self):
        return "Err(DifferentLengthArgs)"


ERR = _Err()


def _codes(s):
    if isinstance(s, str):
        return [ord(c) for c in s]
    return list(s)


def pair(metric, a, b) -> int:
    a, b = _codes(a), _codes(b)
    if metric == "hamming":
        common = min(len(a), len(b))
        return sum(1 for i in range(common) if a[i] != b[i]) + max(len(a), len(b)) - common
    if metric == "postfix":
        a, b = a[::-1], b[::-1]
    n = 0
    while n < len(a) and n < len(b) and a[n] == b[n]:
        n += 1
    return n


def raw_many(metric, query, rows, lens) -> np.ndarray:
    q = np.asarray(_codes(query), dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    n, width = rows.shape
    len1 = len(q)
    w = max(width, len1, 1)
    # query and candidates side by side on w columns; -1 / -2 pad them so that padding never equals padding
    qq = np.full(w, -2, dtype=np.int64)
    cc = np.full((n, w), -1, dtype=np.int64)
    if metric == "postfix":  # right-aligned, read from the end
        qq[:len1] = q[::-1]
        col = np.arange(width)[None, :]
        rev = lens[:, None] - 1 - col
        ok = rev >= 0
        cc[:, :width][ok] = rows[np.nonzero(ok)[0], rev[ok]]
    else:
        qq[:len1] = q
        cc[:, :width] = rows
    eq = cc == qq[None, :]
    common = np.minimum(lens, len1)
    inside = np.arange(w)[None, :] < common[:, None]
    if metric == "hamming":
        return (inside & ~eq).sum(axis=1) + np.maximum(lens, len1) - common
    run = np.cumprod((eq & inside).astype(np.int64), axis=1)  # 1 while every position so far matched
    return run.sum(axis=1)


def op_pair(metric, op, raw, len1, len2, cutoff=None, pad=False):
    if metric == "hamming" and not pad and len1 != len2:
        return ERR  # hamming.rs:232-234, before anything is computed
    maximum = max(len1, len2)  # hamming.rs:166-168, prefix.rs / postfix.rs:48-50
    if metric == "hamming":
        def _distance(_cut):  # hamming.rs:170-187: the cutoff is ignored
            return raw

        def _similarity(cut):  # details/distance.rs:181-211
            if cut is not None and cut > maximum:
                return maximum
            return maximum - _distance(None if cut is None else maximum - cut)
    else:
        def _similarity(_cut):  # prefix.rs / postfix.rs:52-68: the cutoff is ignored
            return raw

        def _distance(cut):  # details/distance.rs:157-179
            return maximum - _similarity(None if cut is None else max(maximum - cut, 0))

    if op == OP_DISTANCE:
        v = _distance(cutoff)
        return None if cutoff is not None and v > cutoff else v
    if op == OP_SIMILARITY:
        v = _similarity(cutoff)
        return None if cutoff is not None and v < cutoff else v
    nd_cut = cutoff
    if op == OP_NORMALIZED_SIMILARITY and cutoff is not None:
        nd_cut = min(1.0 - cutoff + 0.00001, 1.0)  # details/common.rs:4-7 norm_sim_to_norm_dist
    cutoff_distance = None if nd_cut is None else int(math.ceil(maximum * min(max(nd_cut, 0.0), 1.0)))  # :230-236
    d = _distance(cutoff_distance)
    nd = 0.0 if maximum == 0 else d / maximum  # :247-251
    if op == OP_NORMALIZED_DISTANCE:
        return None if cutoff is not None and nd > cutoff else nd
    ns = 1.0 - nd  # :273
    return None if cutoff is not None and ns < cutoff else ns


def ops(metric, op, query, rows, lens, cutoff=None, pad=False, raw=None) -> np.ndarray:
    r = raw_many(metric, query, rows, lens) if raw is None else raw
    len1 = len(_codes(query))
    vals = [op_pair(metric, op, int(ri), len1, int(l2), cutoff, pad) for ri, l2 in zip(r, lens)]
    if op in (OP_DISTANCE, OP_SIMILARITY):
        return np.array([NONE_U32 if v is None else (DIFFERENT_LENGTH_U32 if v is ERR else v) for v in vals], dtype=np.uint32)
    out = np.array([0.0 if (v is None or v is ERR) else v for v in vals], dtype=np.float64)
    bits = out.view(np.uint64)
    for i, v in enumerate(vals):
        if v is None:
            bits[i] = NONE_F64_BITS
        elif v is ERR:
            bits[i] = DIFFERENT_LENGTH_F64_BITS
    return out


def keep(values: np.ndarray) -> np.ndarray:
    """indices of the candidates a `filter_map(|c| scorer.<op>_with_args(c, &args).ok().flatten())` keeps"""
    if values.dtype == np.uint32:
        return np.nonzero((values != NONE_U32) & (values != DIFFERENT_LENGTH_U32))[0]
    return np.nonzero(~np.isnan(values))[0]


def same_bits(got: np.ndarray, exp: np.ndarray) -> np.ndarray:
    """indices where two result vectors differ BY BITS (the two NaNs are different values here)"""
    assert got.dtype == exp.dtype and got.shape == exp.shape, (got.dtype, exp.dtype, got.shape, exp.shape)
    if got.dtype == np.float64:
        return np.nonzero(got.view(np.uint64) != exp.view(np.uint64))[0]
    return np.nonzero(got != exp)[0]
