"""Inputs, catalogue and schedule of tests/call_sequence_check.py (started per mode by tests/test_gpu_call_sequences.py); nothing here touches a GPU, and
tests/test_call_sequences_host.py holds every condition stated below from the CPU side alone.  A helper, not a test file.

What the library keeps between calls -- per (corpus, stream) the top-k scratch with its bound and counters, the score buffer of the scan-plus-one-pass top-k, the
gather temporary, the tile list with its trailer, its pinned report and its survivor count; per corpus the lazily built acceleration structures, take_slot_of,
filter_last_survivors, hint_trust; per comparator d_pm and the `lowered` map; per thread, device or process the result slot, the selection workspace, the streamed
scans' buffer sets, the parked scratch blocks -- may steer speed and nothing else.  So a CALL is a letter with ONE expected value, computed once on the CPU
(oracle/oracle.py, tests/dl_reference.py, tests/textbook.py, or the input itself), and a schedule makes every letter of a corpus follow every letter of that corpus,
itself included; whatever came before, the value is the letter's.

Corpora (each at most ~10 000 candidates: the state protocols need tiles, runs and lists, not volume):
  U   64 x 129 - 27 rows of 64 symbols over the 62 alphanumerics (the 6-bit planes are eligible): an odd tile count, the last tile partial, 129 tiles so that the
      top-k sample pass (tiles >= 8 x RF_TOPK_SAMPLE at 8) and the two-step normalizing road (>= 16 tiles) have something to do.
  R   length-bucketed: runs of 63 and 64 symbols of 42 exact tiles each, a run of 200 symbols of 40 exact tiles (the rows of the 200-symbol queries, made by
      tests/test_gpu_filter._band_rows), 5 rows of every other length 0..70 (mixed tiles, zero-length rows among them); 130 tiles.
  W   `char` elements, lengths 0..32, 312 distinct symbols (the 62 alphanumerics and 250 code points above 255): 254 get an id, the 58 others, planted twice
      each, share the overflow class, so the corpus keeps its raw symbol stream.  W2: a second small wide corpus over a shifted alphabet.  Two `char` queries of
      100 symbols (2 words) put W's top-k on the scan-plus-one-pass road, whose score buffer is kept per (corpus, stream): two queries, so that the scores the
      previous call left there are another query's.  R has one such letter, with the 200-symbol query.
Queries are drawn from the first 50 alphanumerics and planted rows are substituted with the last 12, which no query holds: a copy of the query with e positions
replaced is at Levenshtein distance exactly e and Indel distance exactly 2 e for equal lengths (one more edit, resp. one more symbol, against the rows of 63).

The schedule: per group (U, R, W with W2) a seeded Eulerian circuit of the complete directed graph WITH self-loops -- L x L + 1 calls in which every ordered pair
(a, b), a = b included, is adjacent -- then one seeded walk of CROSS_CALLS calls over all letters, which interleaves the corpora and with them the per-comparator and
per-process state.  R's circuit starts at `take`, so that take runs before and after the first scan that builds the gather maps.

The conditions of the 200-symbol hint letters (`right`: at most a quarter of the rows exceed the hint, `wrong`: at least half) are counted over the rows a hint can
bear on -- those whose length is within max(hint, 31) symbols of the query's, here the run of 200 -- since R must also hold its runs of 63 and 64.  Over the WHOLE
of R some 70 % of the rows are out of a hint's reach, so the sample of a hinted scan without a cutoff (`r.q200.hint8`, `r.q200w.hint8`) finds too few rows resolved,
drops the hint and runs the plain scan: what these two letters hold to the contract is the sample and the decision read from hint_trust.  The hinted road itself
(`hint pass:` in the trace) is taken by `r.q200.hint8<=40` alone, whose cutoff takes the far rows out of the count; it is also the only call that raises
hint_trust, so the two hint letters meet a changed trust only where they follow it -- which the circuit makes them do.  `hint lists:` and its pinned report need a
long query on a single-length corpus, which none of the three is: that road is not run here (tests/multitile_lists_check.py walks it in its `hint` mode).
"""
import functools

import numpy as np

ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
QSYM, SUBS = ALNUM[:50], ALNUM[50:]  # what queries are drawn from / what replaces a query symbol in a planted row
OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY = range(4)
FILTER_BY_INDEX, FILTER_BY_SCORE = 0, 1
NONE32 = np.uint32(0xFFFFFFFF)
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
SEED = 0x5E0CA11
CROSS_CALLS = 400
U_TILES, U_LEN = 129, 64
EDITS = range(13)  # e = 0..12
# planted copies per e: `a` (the main query) few at the small distances, so that its top-k lists hold several scores; `many` (the query whose head most of U
# carries) and the further queries of the multi-query calls the same number at every e
COPIES = {"a": (3, 5, 9) + (12,) * 10, "many": (20,) * 13, "b": (5,) * 13, "c": (5,) * 13, "d": (5,) * 13}
HEAD_SHARE = {"many": 0.60, "a": 0.03, "b": 0.01, "c": 0.01, "d": 0.01}
HINT = 8
LONG_LEN = 200
LONG_W = 100  # the long `char` queries of W


# ---------------------------------------------------------------------------------------------- queries
def substituted(rng, q, length, e):
    """the query cut to `length` with exactly e positions replaced by symbols no query holds"""
    row = np.asarray(q)[:length].copy()
    at = rng.choice(len(row), size=e, replace=False)
    row[at] = SUBS[rng.integers(0, len(SUBS), size=e)]
    return row


def transposed(q, length, at):
    """the query cut to `length` with the symbols at `at`, `at` + 1 swapped: Levenshtein 2, OSA and Damerau-Levenshtein 1"""
    row = np.asarray(q)[:length].copy()
    assert row[at] != row[at + 1]
    row[[at, at + 1]] = row[[at + 1, at]]
    return row


@functools.lru_cache(maxsize=None)
def _short_queries():
    """the five 64-symbol queries as uint8 arrays; their first 8 symbols differ"""
    rng = np.random.default_rng(SEED)
    q = {name: QSYM[rng.integers(0, 50, size=64)] for name in ("a", "many", "b", "c", "d")}
    assert len({bytes(v[:8]) for v in q.values()}) == 5
    return q


def _swap_places(q):
    return [p for p in range(10, 60) if q[p] != q[p + 1]][:6]


# ---------------------------------------------------------------------------------------------- corpora
@functools.lru_cache(maxsize=None)
def corpus_u():
    """{"rows": uint8 [n, 64], "plants": {query: [(index, e)]}, "swaps": the rows that are query `b` with two neighbours swapped,
    "carriers": {query: how many rows carry its first 8 symbols}, "data", "offsets": the rows as the packer takes them}"""
    q = _short_queries()
    rng = np.random.default_rng(SEED + 1)
    n = 64 * U_TILES - 27
    rows = ALNUM[rng.integers(0, 62, size=(n, U_LEN))]
    draw, lo = rng.random(n), 0.0
    for name, share in HEAD_SHARE.items():
        rows[(draw >= lo) & (draw < lo + share), :8] = q[name][:8]
        lo += share
    free = rng.permutation(n).tolist()
    plants = {}
    for name, counts in COPIES.items():
        plants[name] = []
        for e, count in zip(EDITS, counts):
            for _ in range(count):
                i = free.pop()
                rows[i] = substituted(rng, q[name], U_LEN, e)
                plants[name].append((i, e))
    swaps = []
    for at in _swap_places(q["b"]):
        i = free.pop()
        rows[i] = transposed(q["b"], U_LEN, at)
        swaps.append(i)
    rows = np.ascontiguousarray(rows)
    carriers = {name: int(np.count_nonzero((rows[:, :8] == q[name][:8]).all(axis=1))) for name in q}
    return {"rows": rows, "plants": plants, "swaps": swaps, "carriers": carriers, "data": rows.reshape(-1),
            "offsets": np.arange(n + 1, dtype=np.uint64) * np.uint64(U_LEN)}


def band_rows(n, len2, q, share, seed):
    """tests/test_gpu_filter._band_rows(..., kinds=6): near rows (0..12 substitutions, or a symbol more or less near the front) and random ones"""
    import test_gpu_filter as TF

    return TF._band_rows(n, len2, q, share, seed=seed, kinds=6)


@functools.lru_cache(maxsize=None)
def corpus_r():
    """{"data", "offsets", "lens", "plants": {query: [(index, e, length)]}, "take": the index list of the take / lengths letters}"""
    q = _short_queries()
    rng = np.random.default_rng(SEED + 2)
    long_q = queries_long()["q200"]
    lens = [63] * (64 * 42 + 7) + [64] * (64 * 42 + 9) + [LONG_LEN] * (64 * 40 + 13)
    for ln in range(71):
        if ln not in (63, 64):
            lens += [ln] * 5
    lens = np.array(lens, dtype=np.int64)[rng.permutation(len(lens))]
    n = len(lens)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = ALNUM[rng.integers(0, 62, size=int(offsets[-1]))]
    start = offsets[:-1].astype(np.int64)

    def put(i, row):
        assert len(row) == lens[i]
        data[start[i]:start[i] + len(row)] = row

    at_long = np.nonzero(lens == LONG_LEN)[0]
    for i, row in zip(at_long, band_rows(len(at_long), LONG_LEN, long_q, 0.97, SEED + 3)):
        put(i, row)
    free = {ln: rng.permutation(np.nonzero(lens == ln)[0]).tolist() for ln in (63, 64)}
    for ln in (63, 64):  # a small share of head carriers for `a`
        for i in free[ln][-160:]:
            data[start[i]:start[i] + 8] = q["a"][:8]
    plants = {}
    for name, counts in COPIES.items():
        plants[name] = []
        for ln in (64, 63):
            for e, count in zip(EDITS, counts):
                for _ in range(count):
                    i = free[ln].pop()
                    put(i, substituted(rng, q[name], ln, e))
                    plants[name].append((i, e, ln))
    swaps = []
    for j, at in enumerate(_swap_places(q["b"])):
        i = free[64 - j % 2].pop()
        put(i, transposed(q["b"], 64 - j % 2, at))
        swaps.append(i)
    take = rng.integers(0, n, size=300)
    take[::7] = take[0]  # repeats
    take[1] = np.nonzero(lens == 0)[0][0]
    return {"data": np.ascontiguousarray(data), "offsets": offsets, "lens": lens, "plants": plants, "swaps": swaps, "take": take.astype(np.uint64)}


@functools.lru_cache(maxsize=None)
def queries_long():
    rng = np.random.default_rng(SEED + 4)
    long_q = ALNUM[rng.integers(0, 62, size=LONG_LEN)]
    far = long_q.copy()  # the plain-distance letter's query: 30 symbols away from the one the rows are planted around
    far[rng.choice(LONG_LEN, size=30, replace=False)] = SUBS[rng.integers(0, len(SUBS), size=30)]
    return {"q200": long_q.tobytes(), "q200d": far.tobytes(), "q200w": ALNUM[rng.integers(0, 62, size=LONG_LEN)].tobytes()}


def _wide_alphabet(shift):
    return np.concatenate([ALNUM.astype(np.uint32), np.uint32(0x390) + np.uint32(7) * np.arange(shift, shift + 250, dtype=np.uint32)])


def _wide_ragged(rng, n, symbols):
    lens = rng.integers(0, 33, size=n)
    lens[:3] = (0, 32, 24)
    lens[3:63], lens[63:83] = 24, 12  # (room for the planted copies)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = symbols[rng.integers(0, len(symbols), size=int(offsets[-1]))]
    return data, offsets, lens


@functools.lru_cache(maxsize=None)
def corpus_w():
    """W and W2 with their `char` queries: {"W": {...}, "W2": {...}, "queries": {name: uint32 array}}"""
    rng = np.random.default_rng(SEED + 5)
    alphabet = _wide_alphabet(0)
    common, rare = alphabet[:254], alphabet[254:]  # the rare ones are planted twice each: they are the overflow class
    n = 64 * 20 + 11
    data, offsets, lens = _wide_ragged(rng, n, common)
    start = offsets[:-1].astype(np.int64)
    subs = common[224:254]  # what replaces a query symbol in a planted row: no query holds them
    pool = common[62:224]  # `char` symbols above 255 only
    wq = pool[rng.integers(0, len(pool), size=24)]
    wq3 = pool[rng.integers(0, len(pool), size=24)]
    wq4 = pool[rng.integers(0, len(pool), size=12)]
    wqo = pool[rng.integers(0, len(pool), size=24)]
    wqo[[2, 5, 11, 17, 20, 23]] = rare[:6]  # overflow-class symbols
    wq2 = alphabet[rng.permutation(len(alphabet))[:280]]  # more than 254 distinct symbols the corpus stores, overflow symbols among them
    wql = pool[rng.integers(0, len(pool), size=LONG_W)]  # two words: the top-k of these two goes through the kept score buffer
    wql2 = pool[rng.integers(0, len(pool), size=LONG_W)]
    rows24 = rng.permutation(np.nonzero(lens == 24)[0]).tolist()
    rows12 = rng.permutation(np.nonzero(lens == 12)[0]).tolist()
    plants = {}
    for name, query, free in (("wq", wq, rows24), ("wqo", wqo, rows24), ("wq3", wq3, rows24), ("wq4", wq4, rows12)):
        plants[name] = []
        for e in range(min(13, len(query) + 1)):
            i = free.pop()
            row = query.copy()
            row[rng.choice(len(row), size=e, replace=False)] = subs[rng.integers(0, len(subs), size=e)]
            data[start[i]:start[i] + len(row)] = row
            plants[name].append((i, e))
    for name, query in (("wql", wql), ("wql2", wql2)):  # symbols 10..33 of the long query with e replaced: at distance exactly LONG_W - 24 + e
        plants[name] = []
        for e in range(8):
            i = rows24.pop()
            row = query[10:34].copy()
            row[rng.choice(24, size=e, replace=False)] = subs[rng.integers(0, len(subs), size=e)]
            data[start[i]:start[i] + 24] = row
            plants[name].append((i, e))
    planted = {i for v in plants.values() for i, _ in v}
    row_of = np.searchsorted(offsets, np.arange(len(data)), side="right") - 1
    spots = [int(p) for p in rng.permutation(len(data)) if int(row_of[p]) not in planted][:2 * len(rare)]
    data[spots] = np.repeat(rare, 2)
    hist = {int(s): int(np.count_nonzero(data == s)) for s in alphabet}
    assert min(hist[int(s)] for s in common) > max(hist[int(s)] for s in rare)  # the 254 ids go to the common symbols, whatever the order among equals
    take = rng.integers(0, n, size=200)
    take[::5] = take[0]
    w = {"data": np.ascontiguousarray(data.astype(np.uint32)), "offsets": offsets, "lens": lens, "plants": plants, "hist": hist, "ids": {int(s) for s in common},
         "overflow": {int(s) for s in rare}, "take": take.astype(np.uint64)}
    # W2: 64 x 4 + 5 rows over an alphabet shifted by 100 symbols (150 `char` symbols shared with W), with copies of wq and wqo of its own
    rng2 = np.random.default_rng(SEED + 6)
    alphabet2 = _wide_alphabet(100)
    n2 = 64 * 4 + 5
    data2, offsets2, lens2 = _wide_ragged(rng2, n2, alphabet2)
    start2 = offsets2[:-1].astype(np.int64)
    free2 = np.nonzero(lens2 == 24)[0].tolist()
    for j, i in enumerate(free2[:8]):
        row = (wq if j % 2 else wqo).copy()
        row[rng2.choice(24, size=j, replace=False)] = alphabet2[-1 - rng2.integers(0, 20, size=j)]
        data2[start2[i]:start2[i] + 24] = row
    w2 = {"data": np.ascontiguousarray(data2.astype(np.uint32)), "offsets": offsets2, "lens": lens2}
    return {"W": w, "W2": w2, "queries": {"wq": wq, "wq3": wq3, "wq4": wq4, "wqo": wqo, "wq2": wq2, "wql": wql, "wql2": wql2}}


def corpus_input(name):
    """(data, offsets) of corpus `name`, as its packer takes them"""
    if name == "U":
        return corpus_u()["data"], corpus_u()["offsets"]
    if name == "R":
        return corpus_r()["data"], corpus_r()["offsets"]
    return corpus_w()[name]["data"], corpus_w()[name]["offsets"]


def corpus_size(name):
    return len(corpus_input(name)[1]) - 1


def all_queries():
    out = {k: v.tobytes() for k, v in _short_queries().items()}
    out.update(queries_long())
    out.update(corpus_w()["queries"])
    return out


# ---------------------------------------------------------------------------------------------- the CPU side: dense vectors and what follows from them
def u32_of(x):
    return np.where(x == U64MAX, NONE32, x.astype(np.uint32)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def dense(corpus, metric, qname, op, cutoff=None, weights=None):
    """every candidate's value, None = 0xFFFFFFFF (uint32) / NaN (float64): oracle/oracle.py for the byte corpora, tests/dl_reference.py for damerau_levenshtein,
    tests/textbook.py for the `char` corpora"""
    q = all_queries()[qname]
    data, offsets = corpus_input(corpus)
    if corpus in ("W", "W2"):
        return _dense_textbook(corpus, metric, qname, op, cutoff)
    if metric == "damerau_levenshtein":
        import dl_reference as R

        rows, lens = R.ragged_rows(data, offsets)
        return R.ops(op, q, rows, lens, cutoff, dist=_dl_distance(corpus, qname))
    from oracle import oracle as o

    kw = {}
    if cutoff is not None:
        kw["score_cutoff"] = cutoff
    if weights is not None:
        kw["weights"] = weights
    out = getattr(o, metric).BatchComparator(q).many(op, data, offsets, nthreads=8, **kw)
    return u32_of(out) if out.dtype == np.uint64 else out


@functools.lru_cache(maxsize=None)
def _dl_distance(corpus, qname):
    """dl_many in two batches -- the candidates of <= 70 symbols and the longer ones -- so that the short ones are not padded to the longest"""
    import dl_reference as R

    data, offsets = corpus_input(corpus)
    rows, lens = R.ragged_rows(data, offsets)
    out = np.empty(len(lens), dtype=np.int64)
    short = lens <= 70
    out[short] = R.dl_many(all_queries()[qname], rows[short][:, :70], lens[short])
    if (~short).any():
        out[~short] = R.dl_many(all_queries()[qname], rows[~short], lens[~short])
    return out


@functools.lru_cache(maxsize=None)
def _textbook_raw(corpus, metric, qname):
    import textbook as tb

    q = all_queries()[qname]
    q = np.frombuffer(q, dtype=np.uint8).astype(np.uint32) if isinstance(q, bytes) else q
    data, offsets = corpus_input(corpus)
    fn = {"levenshtein": tb.levenshtein_unit, "indel": tb.indel, "lcs_seq": tb.lcs_len, "osa": tb.osa}[metric]
    o = offsets.astype(np.int64)
    return np.array([fn(q, data[o[i]:o[i + 1]]) for i in range(len(o) - 1)], dtype=np.int64)


def _dense_textbook(corpus, metric, qname, op, cutoff):
    raw = _textbook_raw(corpus, metric, qname)
    want = OP_SIMILARITY if metric == "lcs_seq" else OP_DISTANCE  # (lcs_len IS the LCS similarity; the others are distances)
    assert op == want, "the `char` letters use the op the textbook function computes"
    out = raw.astype(np.uint32)
    if cutoff is not None:
        out = np.where(raw >= cutoff, out, NONE32) if op == OP_SIMILARITY else np.where(raw <= cutoff, out, NONE32)
    return out.astype(np.uint32)


def some(vec):
    """(indices uint64, values) of the values that are not None"""
    keep = np.nonzero(~np.isnan(vec))[0] if vec.dtype == np.float64 else np.nonzero(vec != NONE32)[0]
    return keep.astype(np.uint64), vec[keep]


def topk_of(vec, k, desc=False):
    """rfgpu.h: drop None, order by (score, index) -- best first --, keep k: (scores, indices uint64)"""
    idx, val = some(vec)
    key = -val.astype(np.float64) if desc else val.astype(np.float64)
    order = np.lexsort((idx, key))[:k]
    return val[order], idx[order]


def filter_of(vec, by_score=False, desc=False):
    idx, val = some(vec)
    if by_score:
        key = -val.astype(np.float64) if desc else val.astype(np.float64)
        order = np.lexsort((idx, key))
        idx, val = idx[order], val[order]
    return idx, val


def passers(vec):
    return len(some(vec)[0])


def same(got, exp):
    """two canonical values (tuples of arrays) are equal bit for bit; NaN equals NaN"""
    if len(got) != len(exp):
        return False
    for a, b in zip(got, exp):
        a, b = np.asarray(a), np.asarray(b)
        if a.dtype != b.dtype or a.shape != b.shape:
            return False
        if not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
            return False
    return True


def shape_of(value):
    return tuple((np.asarray(a).dtype.str, np.asarray(a).shape) for a in value)


# ---------------------------------------------------------------------------------------------- the catalogue
class Pending:
    """a call whose output is still on the device: read() synchronizes the call's own stream and returns the canonical value"""

    def __init__(self, read):
        self.read = read


class Letter:
    def __init__(self, name, corpus, call, expected, tags=(), check=None, passing=None):
        self.name, self.corpus, self.call, self._expected, self.tags = name, corpus, call, expected, frozenset(tags)
        self.group = "W" if corpus == "W2" else corpus
        self._check = check
        self.passing = passing  # () -> how many candidates pass the letter's cutoff, where it has one (a multi-query letter: one count per query)

    @functools.cached_property
    def expected(self):
        return self._expected()

    def agrees(self, got):
        return self._check(got, self.expected) if self._check else same(got, self.expected)


def _many(corpus, metric, qname, op, tags=(), name=None, **kw):
    cutoff, weights = kw.get("score_cutoff"), kw.get("weights")

    def call(ctx, stream):
        return (ctx.bc(metric, qname).many(op, ctx.corpus[corpus], stream=stream, **kw),)

    def expected():
        return (dense(corpus, metric, qname, op, cutoff, weights),)

    t = set(tags) | ({"cutoff"} if cutoff is not None else set())
    return Letter(name, corpus, call, expected, t, passing=(lambda: passers(dense(corpus, metric, qname, op, cutoff, weights))) if cutoff is not None else None)


def _slot(corpus, metric, qname, op, name, **kw):
    cutoff = kw.get("score_cutoff")

    def call(ctx, stream):
        import rapidfuzz_rs_amd as rf

        slots = ctx.bc(metric, qname).many(op, ctx.corpus[corpus], rf.Args().slot_order(), stream=stream, **kw)
        index = ctx.slot_index[corpus]
        real = index != NONE32
        back = np.full(corpus_size(corpus), np.nan if slots.dtype == np.float64 else NONE32, dtype=slots.dtype)
        seen = np.bincount(index[real], minlength=len(back))
        back[index[real]] = slots[real]
        return (back, (seen == 1).all() & np.ones(1, dtype=bool))

    def expected():
        return (dense(corpus, metric, qname, op, cutoff), np.ones(1, dtype=bool))

    return Letter(name, corpus, call, expected, {"cutoff"} if cutoff is not None else (), passing=(lambda: passers(dense(corpus, metric, qname, op, cutoff))) if cutoff is not None else None)


def _stream(corpus, metric, qname, op, segment_bytes, name, **kw):
    def call(ctx, stream):  # (rf_stream_many_* takes no stream: it runs on streams of its own)
        return (ctx.bc(metric, qname).stream_many(op, ctx.path[corpus], segment_bytes=segment_bytes, **kw),)

    return Letter(name, corpus, call, lambda: (dense(corpus, metric, qname, op, kw.get("score_cutoff")),), {"stream_many"})


def _topk(corpus, metric, qname, k, name, op=OP_DISTANCE, tags=(), **kw):
    cutoff = kw.get("score_cutoff")
    desc = op in (OP_SIMILARITY, OP_NORMALIZED_SIMILARITY)

    def call(ctx, stream):
        return ctx.bc(metric, qname).topk(ctx.corpus[corpus], k, op=op, stream=stream, **kw)

    def expected():
        return topk_of(dense(corpus, metric, qname, op, cutoff), k, desc)

    return Letter(name, corpus, call, expected, set(tags) | {"topk"}, passing=(lambda: passers(dense(corpus, metric, qname, op, cutoff))) if cutoff is not None else None)


def _topk_entries(corpus, metric, qname, k, name):
    def call(ctx, stream):
        out = ctx.entries(k)
        ctx.bc(metric, qname).topk_entries_device(ctx.corpus[corpus], k, out, op=OP_DISTANCE, stream=stream)
        return Pending(lambda: (out.cpu().numpy().view(np.uint64).reshape(-1, 2).copy(),))

    def expected():
        s, i = topk_of(dense(corpus, metric, qname, OP_DISTANCE), k)
        full = np.full((k, 2), U64MAX, dtype=np.uint64)
        full[:len(s), 0], full[:len(s), 1] = s, i
        return (full,)

    return Letter(name, corpus, call, expected, {"topk", "device"})


def _filter(corpus, metric, qname, op, name, order=FILTER_BY_INDEX, capacity=None, tags=(), **kw):
    cutoff = kw["score_cutoff"]
    desc = op in (OP_SIMILARITY, OP_NORMALIZED_SIMILARITY)
    vec = lambda: dense(corpus, metric, qname, op, cutoff)

    def call(ctx, stream):
        bc = ctx.bc(metric, qname)
        idx, val = bc.filter_many(op, ctx.corpus[corpus], capacity=capacity, order=order, stream=stream, **kw)
        return (np.array([bc.last_filter_count], dtype=np.int64), idx, val)

    def expected():
        idx, val = filter_of(vec(), order == FILTER_BY_SCORE, desc)
        return (np.array([len(idx)], dtype=np.int64), idx, val)

    def contract(got, exp):
        """a capacity below the true count: the true count, `capacity` valid pairs of the expected set, in the requested order (ascending index)"""
        count, idx, val = got
        where = np.searchsorted(exp[1], idx)
        return (int(count[0]) == int(exp[0][0]) and len(idx) == capacity and len(val) == capacity and val.dtype == exp[2].dtype and bool(np.all(np.diff(idx.astype(np.int64)) > 0)) and
                bool(np.all(where < len(exp[1]))) and bool(np.array_equal(exp[1][np.minimum(where, len(exp[1]) - 1)], idx)) and bool(np.array_equal(exp[2][np.minimum(where, len(exp[1]) - 1)], val)))

    def count_only(got, exp):
        return int(got[0][0]) == int(exp[0][0]) and len(got[1]) == 0 and len(got[2]) == 0

    check = None if capacity is None else (count_only if capacity == 0 else contract)
    return Letter(name, corpus, call, expected, set(tags) | {"filter", "cutoff"}, check=check, passing=lambda: passers(vec()))


MULTI = ("a", "many", "b", "c", "d")  # five queries: the fused passes take them 4 (or 2) at a time, one is the odd one left over


def _many_multi(corpus, metric, op, name):
    def call(ctx, stream):
        import rapidfuzz_rs_amd as rf

        cs = [ctx.bc(metric, q) for q in MULTI]
        return (getattr(rf.distance, metric).BatchComparator.many_multi(cs, op, ctx.corpus[corpus], stream=stream),)

    return Letter(name, corpus, call, lambda: (np.stack([dense(corpus, metric, q, op) for q in MULTI]),), {"multi"})


def _topk_multi(corpus, metric, op, k, name):
    desc = op in (OP_SIMILARITY, OP_NORMALIZED_SIMILARITY)

    def call(ctx, stream):
        import rapidfuzz_rs_amd as rf

        cs = [ctx.bc(metric, q) for q in MULTI]
        pairs = getattr(rf.distance, metric).BatchComparator.topk_multi(cs, ctx.corpus[corpus], k, op=op, stream=stream)
        return tuple(x for pair in pairs for x in pair)

    return Letter(name, corpus, call, lambda: tuple(x for q in MULTI for x in topk_of(dense(corpus, metric, q, op), k, desc)), {"multi", "topk"})


def _filter_multi(corpus, metric, op, cutoff, name):
    def call(ctx, stream):
        import rapidfuzz_rs_amd as rf

        cls = getattr(rf.distance, metric).BatchComparator
        pairs = cls.filter_multi([ctx.bc(metric, q) for q in MULTI], op, ctx.corpus[corpus], capacity=1024, stream=stream, score_cutoff=cutoff)
        return (np.array(cls.last_filter_counts, dtype=np.int64),) + tuple(x for pair in pairs for x in pair)

    def expected():
        pairs = [filter_of(dense(corpus, metric, q, op, cutoff)) for q in MULTI]
        return (np.array([len(p[0]) for p in pairs], dtype=np.int64),) + tuple(x for pair in pairs for x in pair)

    return Letter(name, corpus, call, expected, {"multi", "filter", "cutoff"}, passing=lambda: [passers(dense(corpus, metric, q, op, cutoff)) for q in MULTI])


def _take(corpus, name):
    def indices():
        return (corpus_r() if corpus == "R" else corpus_w()[corpus])["take"]

    def call(ctx, stream):
        return ctx.corpus[corpus].take(indices(), stream=stream)

    def expected():
        data, offsets = corpus_input(corpus)
        o = offsets.astype(np.int64)
        parts = [data[o[i]:o[i + 1]] for i in indices().astype(np.int64)]
        out = np.zeros(len(parts) + 1, dtype=np.uint64)
        out[1:] = np.cumsum([len(p) for p in parts])
        return (np.concatenate(parts).astype(data.dtype), out)

    return Letter(name, corpus, call, expected, {"take"})


def _lengths(corpus, name):
    def indices():
        return (corpus_r() if corpus == "R" else corpus_w()[corpus])["take"]

    def call(ctx, stream):
        return (ctx.corpus[corpus].lengths(indices(), stream=stream),)

    return Letter(name, corpus, call, lambda: (np.diff(corpus_input(corpus)[1].astype(np.int64))[indices().astype(np.int64)].astype(np.uint32),), {"take"})


NOTHING = (np.zeros(0, dtype=np.uint8),)


def _release(corpus, name):
    def call(ctx, stream):
        from rapidfuzz_rs_amd import _native as N

        assert N.lib().rf_release_caches() == N.RF_OK
        return NOTHING

    return Letter(name, corpus, call, lambda: NOTHING, {"novalue"})


def _refused(corpus, name, attempt, status):
    """a documented refusal, decided on the host before a device is touched: the value is the status"""

    def call(ctx, stream):
        import rapidfuzz_rs_amd as rf

        try:
            attempt(ctx, stream)
        except rf.RfError as e:
            return (np.array([e.status], dtype=np.int64),)
        return (np.array([0], dtype=np.int64),)

    return Letter(name, corpus, call, lambda: (np.array([status], dtype=np.int64),), {"refused"})


RF_ERR_INVALID_ARG, RF_ERR_UNSUPPORTED = 1, 3


def _refuse_slot_overflow(ctx, stream):
    import rapidfuzz_rs_amd as rf

    ctx.bc("levenshtein", "wqo").many(OP_DISTANCE, ctx.corpus["W"], rf.Args().slot_order(), stream=stream)


def _refuse_jaro_topk_multi(ctx, stream):
    import rapidfuzz_rs_amd as rf

    rf.distance.levenshtein.BatchComparator.topk_multi([ctx.bc("jaro", "wq"), ctx.bc("jaro", "wq3")], ctx.corpus["W"], 16, op=OP_DISTANCE, stream=stream)


def _refuse_too_many_symbols(ctx, stream):
    ctx.bc("levenshtein", "wq2").many(OP_DISTANCE, ctx.corpus["W"], stream=stream)


@functools.lru_cache(maxsize=None)
def catalogue():
    """{group: [Letter]}: 24 letters on U, 24 on R, 21 on W with W2"""
    lev, ind = "levenshtein", "indel"
    D, S, ND, NS = OP_DISTANCE, OP_SIMILARITY, OP_NORMALIZED_DISTANCE, OP_NORMALIZED_SIMILARITY
    U = [
        _many("U", lev, "a", D, name="u.lev"),
        _many("U", lev, "a", D, name="u.lev<=3", score_cutoff=3),
        _many("U", lev, "many", D, name="u.lev<=0.many", score_cutoff=0),
        _many("U", lev, "a", NS, name="u.lev.nsim>=0.9", score_cutoff=0.9),
        _many("U", ind, "a", D, name="u.indel", tags={"data6"}),
        _many("U", ind, "a", NS, name="u.indel.nsim"),
        _many("U", "osa", "b", D, name="u.osa.b"),
        _topk("U", lev, "a", 1, "u.top1"),
        _topk("U", lev, "a", 16, "u.top16"),
        _topk("U", lev, "a", 64, "u.top64"),
        _topk("U", lev, "a", 65, "u.top65"),
        _topk("U", lev, "a", 300, "u.top300"),
        _topk("U", lev, "a", 24, "u.top24<=3", score_cutoff=3),
        _topk("U", lev, "a", 8, "u.top8.hint2", score_hint=2),
        _topk("U", lev, "a", 16, "u.top16.nsim", op=NS),
        _topk("U", lev, "a", 64, "u.top64<=2.short", tags={"short"}, score_cutoff=2),
        _topk_entries("U", lev, "b", 16, "u.top16.entries.b"),
        _filter("U", lev, "a", D, "u.filter<=3.few", tags={"few"}, score_cutoff=3),
        _filter("U", lev, "many", D, "u.filter<=3.many", tags={"many"}, score_cutoff=3),
        _filter("U", lev, "many", D, "u.filter<=3.many.cap50", capacity=50, tags={"cap50"}, score_cutoff=3),
        _filter("U", lev, "a", D, "u.filter<=5.cap0", capacity=0, score_cutoff=5),
        _filter("U", lev, "a", D, "u.filter<=4.by_score", order=FILTER_BY_SCORE, score_cutoff=4),
        _stream("U", lev, "c", D, 32 << 10, "u.stream.c"),
        _release("U", "u.release"),
    ]
    R = [
        _take("R", "r.take"),
        _lengths("R", "r.lengths"),
        _topk("R", lev, "q200", 16, "r.top16.q200", tags={"via-scores"}),  # (the plain Levenshtein scan of R: r.many_multi, r.lev.w123, r.q200d)
        _many("R", lev, "a", D, name="r.lev<=3", score_cutoff=3),
        _many("R", ind, "a", D, name="r.indel", tags={"gather"}),
        _many("R", "jaro_winkler", "a", S, name="r.jw"),
        _many("R", "damerau_levenshtein", "b", D, name="r.dl.b"),
        _many("R", lev, "a", D, name="r.lev.w123", weights=(1, 2, 3)),
        _many("R", lev, "q200d", D, name="r.q200d"),
        _many("R", lev, "q200", D, name="r.q200<=8", score_cutoff=8),
        _many("R", lev, "q200", NS, name="r.q200.nsim>=0.9", score_cutoff=0.9),
        _many("R", lev, "q200", D, name="r.q200.hint8", tags={"hint-right"}, score_hint=HINT),
        _many("R", lev, "q200w", D, name="r.q200w.hint8", tags={"hint-wrong"}, score_hint=HINT),
        _many("R", lev, "q200", D, name="r.q200.hint8<=40", score_hint=HINT, score_cutoff=40),
        _slot("R", lev, "a", D, "r.slots<=5", score_cutoff=5),
        _slot("R", ind, "c", ND, "r.slots.indel.ndist.c"),
        _many_multi("R", lev, D, "r.many_multi"),
        _topk_multi("R", lev, D, 16, "r.topk_multi"),
        _topk_multi("R", lev, NS, 16, "r.topk_multi.nsim"),
        _filter_multi("R", lev, D, 3, "r.filter_multi<=3"),
        _filter_multi("R", lev, NS, 0.9, "r.filter_multi.nsim>=0.9"),
        _filter("R", ind, "a", NS, "r.filter.indel.nsim>=0.8", score_cutoff=0.8),
        _stream("R", lev, "d", D, 0, "r.stream.d"),
        _release("R", "r.release"),
    ]
    W = [
        _many("W", lev, "wq", D, name="w.lev"),
        _many("W", lev, "wq", D, name="w.lev<=3", score_cutoff=3),
        _many("W", lev, "wqo", D, name="w.lev.overflow"),
        _many("W", ind, "wq", D, name="w.indel"),
        _many("W", "lcs_seq", "wq", S, name="w.lcs.sim"),
        _many("W", "osa", "wq4", D, name="w.osa.wq4"),
        _many("W", lev, "a", D, name="w.lev.bytes.a"),  # (the comparators of u.lev / r.lev<=3 and u.indel / r.indel)
        _many("W", ind, "a", D, name="w.indel.bytes.a"),
        _many("W2", lev, "wq", D, name="w2.lev"),
        _many("W2", lev, "wqo", D, name="w2.lev.overflow"),
        _topk("W", lev, "wq", 16, "w.top16"),
        _topk("W", lev, "wql", 16, "w.top16.wql", tags={"via-scores"}),
        _topk("W", lev, "wql2", 5, "w.top5.wql2", tags={"via-scores"}),
        _filter("W", lev, "wqo", D, "w.filter<=3.overflow", score_cutoff=3),
        _take("W", "w.take"),
        _stream("W", lev, "wq3", D, 32 << 10, "w.stream.wq3"),
        _stream("W", ind, "wqo", D, 0, "w.stream.indel.overflow"),
        _refused("W", "w.refused.slot_order", _refuse_slot_overflow, RF_ERR_UNSUPPORTED),
        _refused("W", "w.refused.jaro_topk_multi", _refuse_jaro_topk_multi, RF_ERR_INVALID_ARG),
        _refused("W", "w.refused.symbols", _refuse_too_many_symbols, RF_ERR_UNSUPPORTED),
        _release("W", "w.release"),
    ]
    return {"U": U, "R": R, "W": W}


def letters():
    return {lt.name: lt for group in catalogue().values() for lt in group}


# ---------------------------------------------------------------------------------------------- the schedule
def euler_circuit(names, seed, first=None):
    """a circuit through every ordered pair of `names`, (a, a) included: len(names)^2 + 1 entries, the same for the same seed (Hierholzer over shuffled edge lists)"""
    rng = np.random.default_rng(seed)
    L = len(names)
    out_edges = {a: [names[j] for j in rng.permutation(L)] for a in names}
    start = names[0] if first is None else first
    stack, circuit = [start], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == L * L + 1 and circuit[0] == start == circuit[-1]
    return circuit


def schedule(seed=SEED):
    """[(part, letter name)]: the three circuits, then the walk over all letters"""
    cat = catalogue()
    out = []
    for j, group in enumerate(("U", "R", "W")):
        names = [lt.name for lt in cat[group]]
        out += [(group, nm) for nm in euler_circuit(names, seed + 17 * j, first="r.take" if group == "R" else None)]
    every = [lt.name for group in ("U", "R", "W") for lt in cat[group]]
    rng = np.random.default_rng(seed + 99)
    out += [("cross", every[int(j)]) for j in rng.integers(0, len(every), size=CROSS_CALLS)]
    return out
