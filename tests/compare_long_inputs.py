"""The long-string cases that tests/test_compare_long_inputs.py (no GPU), tests/test_gpu_compare_long.py and tests/compare_long_check.py share: hamming,
prefix and postfix (rf_compare.hip) at their length limits.  A helper, not a test file.

A case is a corpus and the queries it was built around: `case(name)` -> Case(name, queries {label: codes}, cands [codes], wide), made once per process and
handed out read-only, like `rows_lens(name)` (the [n, max_len] form tests/compare_reference.py takes) and `raw(name, metric, label)` (the reference's raw
values, which every op and every cutoff of a test is derived from).  Strings are numpy arrays of symbol CODES (uint8, or uint32 for the `char` cases).

Candidate i is related to query (i // 6 mod #queries) in the way i mod 6: 0 a shared prefix of random length, 1 a shared suffix of random length, 2 the query
left-aligned with 0..3 symbols replaced, 3 the query right-aligned with 0..3 symbols replaced, 4 and 5 unrelated.  Every corpus holds 64 k + r candidates,
1 <= r <= 63.  The planted tiles (`one_live`, `depths`, `full`) are 64 consecutive candidates of the query's length: a single-length corpus keeps them as
its tiles in this order, and a ragged corpus keeps whole tiles of one length in input order (tests/compare_long_check.py asserts that from the host layout).

Hamming's unrolled loop runs (nch - 1) // 4 times over nch = ceil(min(len1, len2) / 16) chunk rows and leaves nch - 4 x that many rows to the tail.  The
lengths of the issue -- nch in {5, 6, 7, 8, 9, 12, 13, 63, 64, 256, 257} -- give the tail 2 rows only after ONE pass (nch 6), so nch 10 and 11 are added:
with them the tail runs with 1, 2, 3 and 4 rows after two passes or more.

tests/test_compare_long_inputs.py holds all of this from the reference alone; measured there: 8 s for the whole file on one CPU core, 4.6 s of it in the
test that first needs the raw values of every case (the reference over the longest cases)."""
import functools
from typing import NamedTuple

import numpy as np

import compare_reference as R

SYM = 20
BASE = 97
QUERY_LENS = [65, 80, 81, 128, 129, 193, 1000, 4096, 4097]
HAMMING_EXTRA = [112, 160, 176, 192, 1024]  # equal-length corpora only: chunk-row counts 7, 10, 11, 12 and 64
HAMMING_NCH = {5, 6, 7, 8, 9, 12, 13, 63, 64, 256, 257}
LDS_LAST_DEFAULT = 49_104  # (4 + ceil(len1 / 4) + 8) * 4 bytes = 48 KiB exactly: the last query on the default dynamic-LDS limit
LDS_FIRST_ATTRIBUTE = 49_105
QUERY_LIMIT = 150_000
SHIFT_LENGTHS = list(range(200, 216))


class Case(NamedTuple):
    name: str
    queries: dict  # label -> codes
    cands: list
    wide: bool


def n_candidates(length):
    return 64 * 5 + 7 if length < 1000 else 64 + 3


def nch(m):
    return (m + 15) // 16


def hamming_passes(m):
    """(passes of the four-rows-in-flight loop, rows left to the tail) for a common length m"""
    passes = (nch(m) - 1) // 4 if nch(m) > 4 else 0
    return passes, nch(m) - 4 * passes


# ------------------------------------------------------------------------------------------------ strings, in symbol indices 0 .. sym - 1
def _other(v, sym):
    return (v + 1) % sym


def near(rng, q, length, how, sym):
    fill = rng.integers(sym, size=length)
    m = min(len(q), length)
    if m == 0 or how >= 4:
        return fill
    if how == 0:
        p = int(rng.integers(0, m + 1))
        fill[:p] = q[:p]
        if p < m and fill[p] == q[p]:
            fill[p] = _other(q[p], sym)
    elif how == 1:
        p = int(rng.integers(0, m + 1))
        if p:
            fill[length - p:] = q[len(q) - p:]
        if p < m and fill[length - p - 1] == q[len(q) - p - 1]:
            fill[length - p - 1] = _other(q[len(q) - p - 1], sym)
    elif how == 2:
        fill[:m] = q[:m]
        for pos in rng.integers(0, m, size=int(rng.integers(0, 4))):
            fill[pos] = _other(q[pos], sym)
    else:
        fill[length - m:] = q[len(q) - m:]
        for pos in rng.integers(0, m, size=int(rng.integers(0, 4))):
            fill[length - m + pos] = _other(q[len(q) - m + pos], sym)
    return fill


def related(rng, queries, lengths, sym):
    qs = [q for q in queries if len(q)]
    return [near(rng, qs[(i // 6) % len(qs)], int(L), i % 6, sym) for i, L in enumerate(lengths)]


def one_live(q, lane, metric, sym):
    """64 copies of the query; all but `lane` differ from it in the first symbol (prefix) / the last one (postfix)"""
    tile = [q.copy() for _ in range(64)]
    pos = 0 if metric == "prefix" else len(q) - 1
    for i, c in enumerate(tile):
        if i != lane:
            c[pos] = _other(q[pos], sym)
    return tile


def depths(q, step, metric, sym):
    """64 copies of the query; copy i matches i * step + 1 symbols from the front (prefix) / from the end (postfix), then differs"""
    tile = [q.copy() for _ in range(64)]
    for i, c in enumerate(tile):
        p = i * step + 1
        assert p < len(q)
        pos = p if metric == "prefix" else len(q) - 1 - p
        c[pos] = _other(q[pos], sym)
    return tile


def full(q):
    return [q.copy() for _ in range(64)]


def planted_tiles(q, step, sym, lanes=(37, 5)):
    """the six tiles the early-out tests are about, in the order a wavefront of a one-workgroup launch meets them (tile t, then t + 4)"""
    return (one_live(q, lanes[0], "prefix", sym) + one_live(q, lanes[1], "postfix", sym) + depths(q, step, "prefix", sym) + depths(q, step, "postfix", sym)
            + full(q) + full(q))


# ------------------------------------------------------------------------------------------------ the cases
def _bytes_case(name, rng, qlens, lengths, sym=SYM, base=BASE, head=None, shuffle=True):
    """queries of these lengths, candidates of these lengths related to them; `head(queries)` -> candidates (indices) that go first, unshuffled"""
    queries = {L: rng.integers(sym, size=L) for L in qlens}
    first = head(queries) if head else []
    lengths = [int(v) for v in lengths]
    if shuffle:
        lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    cands = first + related(rng, list(queries.values()), lengths, sym)
    assert 1 <= len(cands) % 64 <= 63, (name, len(cands))
    return Case(name, {k: (base + v).astype(np.uint8) for k, v in queries.items()}, [(base + c).astype(np.uint8) for c in cands], False)


def _ragged_lengths(qlen):
    if qlen >= 1000:
        return [qlen] * 64 + [qlen - 1, qlen + 1, qlen - 17]
    around = [qlen - 33, qlen - 17, qlen - 16, qlen - 15, qlen - 1, qlen + 1, qlen + 15, qlen + 16, qlen + 17, qlen + 33]
    lengths = [qlen] * 70 + [qlen - 16] * 66 + [qlen + 1] * 65 + around * 12
    return lengths + [qlen - 2] * (n_candidates(qlen) - len(lengths))


def _shift_head(queries):
    return planted_tiles(queries[300], 4, SYM)


def _alphabet_case(name, rng, length, n, alphabet, absent, overflow=None):
    """a `char` corpus over `alphabet` (u32 codes); the query "absent" is the main one with a symbol the corpus does not hold.  With `overflow` (indices of
    symbols that each occur once or twice): two of them sit in the query, and the last three candidates are the query and the query with ONE of them replaced
    by another overflow-class symbol, near the front and near the end."""
    sym = len(alphabet) if overflow is None else overflow[0]  # (the random text draws from the common symbols only)
    q = rng.integers(sym, size=length)
    equal = 70 if n > 100 else 40
    lengths = [length] * equal + [int(v) for v in rng.integers(max(length - 40, 0), length + 40, size=n - equal - (3 if overflow else 0))]
    cands = related(rng, [q], lengths, sym)  # (related to the query BEFORE it takes its two rare symbols: these stay rare)
    if overflow:
        # Ids go to the 254 most frequent symbols.  The first four rare ones occur three times each and take the last four ids; every other one occurs
        # once or twice and is lumped -- overflow[5..8], which decide the last three candidates, among them.
        for j, r in enumerate(overflow):
            for k in range(3 if j < 4 else (0 if 5 <= j <= 8 else 1)):
                c = cands[(j * 7 + k * 3) % len(cands)]
                c[(j + k) % 5] = r
        q[3], q[length - 4] = overflow[5], overflow[6]
        front, back = q.copy(), q.copy()
        front[3] = overflow[7]  # the query with ONE overflow-class symbol replaced by another: the two must be told apart
        back[length - 4] = overflow[8]
        cands += [q.copy(), front, back]
    assert 1 <= len(cands) % 64 <= 63, (name, len(cands))
    alphabet = np.asarray(alphabet, dtype=np.uint32)
    qa = alphabet[q]
    qabs = np.concatenate([qa[:10], np.array([absent], dtype=np.uint32), qa[10:]])
    return Case(name, {"main": qa, "absent": qabs}, [alphabet[c] for c in cands], True)


def _all256_case(name, rng, length):
    q = rng.integers(256, size=length)
    q[0], q[length - 1], q[length // 2], q[length // 2 + 1] = 0x00, 0xFF, 0xFF, 0x00
    lengths = [length] * 70 + [int(v) for v in rng.integers(max(length - 30, 1), length + 30, size=n_candidates(length) - 70 - 8)]
    lengths = [lengths[i] for i in rng.permutation(len(lengths))]
    cands = related(rng, [q], lengths, 256)
    for first, last in ((0x00, 0xFF), (0xFF, 0x00), (0x00, 0x00), (0xFF, 0xFF)):  # the two bytes at first and last positions, on copies and on noise
        c = q.copy()
        c[0], c[-1] = first, last
        cands.append(c)
        c = rng.integers(256, size=length + 5)
        c[0], c[-1] = first, last
        cands.append(c)
    seen = set(np.concatenate(cands).tolist())  # every byte value occurs:
    spare = [i for i, c in enumerate(cands[:-8]) if len(c) > 8 and i % 6 >= 4]  # unrelated rows take the values that did not come up
    for k, v in enumerate(sorted(set(range(256)) - seen)):
        cands[spare[k % len(spare)]][3 + k // len(spare)] = v
    assert 1 <= len(cands) % 64 <= 63, (name, len(cands))
    return Case(name, {length: q.astype(np.uint8)}, [c.astype(np.uint8) for c in cands], False)


def _build(name):
    kind, _, rest = name.partition("-")
    rng = np.random.default_rng([ord(ch) for ch in name])
    if kind == "single":  # single-<query length>-<candidate length>
        qlen, len2 = (int(v) for v in rest.split("-"))
        return _bytes_case(name, rng, [qlen], [len2] * n_candidates(len2))
    if kind == "ragged":  # ragged-<query length>: an exact tile of the query's length (and, below 1000, of two more), the rest mixed
        qlen = int(rest)
        return _bytes_case(name, rng, [qlen], _ragged_lengths(qlen))
    if kind == "shift":  # postfix's shifts: 200..215 and 300; the planted tiles lead the 300-symbol group
        lengths = [L for L in SHIFT_LENGTHS for _ in range(64 * 2 + 3)]
        lengths = [lengths[i] for i in rng.permutation(len(lengths))] + [300] * (64 * 2 + 3)
        return _bytes_case(name, rng, [300, 230, 190, 23], lengths, head=_shift_head, shuffle=False)
    if kind == "mirror":  # a long query over candidates of at most 23 symbols
        return _bytes_case(name, rng, [310], [L for L in range(0, 24) for _ in range(13)] + [23] * 15)
    if kind == "earlyout":  # single length 4100: the one-live-lane tiles and the depth tiles
        return _bytes_case(name, rng, [4100], [4100] * 5, head=lambda qs: planted_tiles(qs[4100], 60, SYM)[: 64 * 4], shuffle=False)
    if kind == "mtsingle":  # single length 1000, 64 * 9 + 5: the planted tiles are tiles 0..5
        return _bytes_case(name, rng, [1000], [1000] * (64 * 3 + 5), head=lambda qs: planted_tiles(qs[1000], 15, SYM), shuffle=False)
    if kind == "ldslong":  # ldslong-<query length>: 67 candidates about as long as the query
        qlen = int(rest)
        return _bytes_case(name, rng, [qlen, 23], [qlen] * 64 + [qlen - 1, qlen + 1, qlen - 100])
    if kind == "ldsshort":
        return _bytes_case(name, rng, [LDS_LAST_DEFAULT, LDS_FIRST_ATTRIBUTE, 23], [23] * 64 + list(range(0, 67)) + [40] * 4)
    if kind == "limit":
        return _bytes_case(name, rng, [QUERY_LIMIT], [QUERY_LIMIT] * 64 + [QUERY_LIMIT - 1, QUERY_LIMIT + 1, QUERY_LIMIT - 16])
    if kind == "longcand":  # candidates the device packer leaves to the host one, among short ones
        return _bytes_case(name, rng, [23, 65_536], [23] * 64 + [int(v) for v in rng.integers(0, 67, size=130)] + [65_535, 65_536, 70_000])
    if kind == "road":  # the roads at a 600-symbol query; 0, 16 and 49 105 symbols ride along in the multi calls
        lengths = [600] * 70 + [584] * 66 + [601] * 65 + [int(v) for v in rng.integers(560, 640, size=126)]
        return _bytes_case(name, rng, [600, 0, 16, LDS_FIRST_ATTRIBUTE], lengths)
    if kind == "order":  # the order-of-calls corpus: short candidates and three as long as the long query
        lengths = [23] * 70 + [int(v) for v in rng.integers(0, 67, size=120)] + [LDS_FIRST_ATTRIBUTE] * 2 + [LDS_FIRST_ATTRIBUTE - 5]
        return _bytes_case(name, rng, [23, LDS_FIRST_ATTRIBUTE], lengths)
    if kind == "char40":  # char40-<length>: 40 symbols above 255
        length = int(rest)
        return _alphabet_case(name, rng, length, n_candidates(length), list(range(0x430, 0x430 + 38)) + [0x9999, 0x1F600], absent=0x4E2D)
    if kind == "charover":  # charover-<length>: 250 common symbols and 40 that occur once or twice -- more than 254, so an overflow class
        length = int(rest)
        return _alphabet_case(name, rng, length, n_candidates(length), list(range(0x400, 0x400 + 250)) + list(range(0x3000, 0x3000 + 40)), absent=0x4E2D,
                              overflow=list(range(250, 290)))
    if kind == "all256":  # all256-<length>: every byte value, 0x00 and 0xFF at the edges
        return _all256_case(name, rng, int(rest))
    raise KeyError(name)


def length_cases():
    """the (query length, corpus) grid of the lengths test, by query length"""
    out = {}
    for q in QUERY_LENS:
        out[q] = [f"single-{q}-{L}" for L in (q - 1, q, q + 1)] + [f"ragged-{q}"]
    return out


EXTRA_CASES = [f"single-{m}-{m}" for m in HAMMING_EXTRA]
SPECIAL_CASES = ["shift", "mirror", "earlyout", "mtsingle", f"ldslong-{LDS_LAST_DEFAULT}", f"ldslong-{LDS_FIRST_ATTRIBUTE}", "ldsshort", "limit", "longcand", "road",
                 "order", "char40-300", "char40-5000", "charover-300", "charover-5000", "all256-40", "all256-300"]


def all_cases():
    return [n for names in length_cases().values() for n in names] + EXTRA_CASES + SPECIAL_CASES


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    c = _build(name)
    for a in list(c.queries.values()) + c.cands:
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=4)  # (the rows of the long cases are tens of megabytes as int64: a few stay)
def rows_lens(name):
    rows, lens = R.pad_rows(case(name).cands)
    rows.setflags(write=False)
    lens.setflags(write=False)
    return rows, lens


@functools.lru_cache(maxsize=None)
def raw(name, metric, label):
    rows, lens = rows_lens(name)
    out = R.raw_many(metric, case(name).queries[label], rows, lens)
    out.setflags(write=False)
    return out


def raw_of(name, metric, query):
    """the same for a query that is no member of the case"""
    rows, lens = rows_lens(name)
    return R.raw_many(metric, query, rows, lens)
