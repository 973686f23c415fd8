"""Run by tests/test_gpu_symbol_edges.py in child processes with RF_TRACE_PLAN=1 RF_PACK_TIMING=1 and each leg's switches (the library reads its switches once per
process); the generators on top are also what tests/test_symbol_edge_inputs.py checks on the host.

The 6-bit payload, the 6-bit head plane and the conflict-free Jaro table exist only while the largest STORED symbol code (after the frequency-rank renaming of
make_sigma, rf_api.hip) is below a bound of its own: DESIGN.md section 4 has the table of bounds and the leg below that guards each row.  The other tests run these
roads at 62 distinct symbols and at 70, with queries made of corpus symbols only.  Here: D = 62, 63, 64, 65 distinct symbols -- the first D of ALNUM + bytes 33..40,
every one planted, the D-th strictly rarest so that its code is D - 1 -- and queries that hold the bytes whose codes are 63 (the fill code's table row), 64 and 65
(rows a 6-bit code cannot name), read from the corpus' own sigma through rapidfuzz_rs_amd.corpus.host_layout.  A symbol that is absent from the corpus still has a
code: make_sigma is a stable sort by count, so the absent bytes follow the present ones in ascending byte order (D = 62: byte 1 owns row 63; D = 63: byte 0 does).

Every value is compared with the oracle.  Which road a call took is read from its `[rf plan] raw=...` line (data6=, heads8=, heads6=) and compared with the
expect_*() functions below, which know D and the length and nothing of the library; a structure that must not exist must print no `[rf accel]` line either.  So a
silent fall-back to the 8-bit kernels fails, and so does a structure that is built where it cannot represent a stored symbol.  (data6=1 says that the plan holds the
structure; that launch_state then takes the asm scan over it also needs the A/B switches of rf_scan.hip at their defaults, which main() asserts.)

argv[1] is the leg:
  payload   RF_PACK6_MIN_TILES=1: single-length corpora of 64 (whole chunks), 57 (a 7-column fill) and 7 (one partial chunk) symbols; Indel and LCS, the four ops,
            three normalized cutoffs that keep the streaming scan (the f64 table stream_asm_f64_table), fuzz.RatioBatchComparator; queries of 20 (32-bit kernels)
            and 40 (64-bit kernels) symbols of the four families below.
  bucketed  RF_PACK6_MIN_TILES=1: lengths 0..80 (exact and mixed tiles); the u32 ops take the 6-bit tiles kernels for D <= 64, the f64 ops and Levenshtein (the
            control) never do.
  heads     RF_HEAD8_MIN=1 RF_BAND_FILTER=1: Levenshtein and OSA distance_many under cutoffs 0..3 and filter_many, queries of 40 and 64 symbols over rows of the
            same length whose planted rows have their edits in the first 8 symbols, on and around the rarest symbol.  With RF_HEAD6=0: no 6-bit plane at any D.
  jaro      RF_JARO_PRIV=1 (and unset): Jaro and Jaro-Winkler similarity_many over rows of 64, D = 63, 64, 65.
  norename  RF_NO_RENAME=1 RF_PACK6_MIN_TILES=1 RF_HEAD8_MIN=1 RF_BAND_FILTER=1: the stored code is the byte itself; ten-symbol alphabets whose largest byte is 62,
            63 and 64, rows of 57 and 64; Indel, and Levenshtein under cutoff 2 through the head plane; every query holds byte 63.
  saveload  RF_PACK6_MIN_TILES=1: the D = 63 corpus of 57 symbols after Corpus.save / Corpus.load: the bound is computed again, the roads must be the same.

Query families, all derived from one base query of corpus symbols that holds the rarest symbol at positions 3 and 12:
  a  the base query
  b  a, with the code-63 byte at position 1 and as a run of 7 at the end (8 positions): behind a 57-symbol candidate a live fill row adds up to 7 to the LCS
  c  a, with the code-64 and code-65 bytes and byte 255 mixed in
  d  nothing but the code-63 byte

One line per corpus with the number of checks; a line per failing check; `DIGEST <sha256 of every result vector>` and `FAILURES n` last; exit status 0 = all equal.
A mismatch is a value, and so is a call that its launcher refuses before anything runs: the leg runs to its end.  A HIP error raises and ends the process.

Planted errors tried on an MI355X (not committed), every leg run against each; groups with failures / checks that failed:
  launch_stream_asm without `a.flags |= 8u`: payload 4 groups (D = 62 and 63 over rows of 57 and 7: 25 / 29 of 120 checks each, all under the queries b20 and d20 --
      every value of a row too large by the fill columns, e.g. Indel distance 57 where 71 is due), norename 1 (largest byte 62, rows of 57: 12 of 30), saveload 1
      (12 of 56).  The queries of 40 symbols (the 64-bit kernel shifts the partial chunk) and every other leg stay green.
  `63u` as `64u` in corpus_data6: payload 2 groups (D = 64 over rows of 57 and 7), norename 1 (largest byte 63, rows of 57): every call shows data6=1 where 0 is due
      and the `[rf accel] 6-bit payload` line is printed; the calls of the queries of 20 symbols are refused by launch_stream_asm's own guard (RF_ERR_UNSUPPORTED,
      counted as failed checks), those of 40 symbols return the right values over the structure that should not exist.
  `>= 64u` as `> 64u` in corpus_head6_plane: heads 2 groups (D = 65, rows of 40 and 64: 49 of 64 checks each -- heads6=1 on every distance_many call, the
      `[rf accel]` line, and None where the planted rows that hold the rarest symbol in their head are due, e.g. candidate 100 at cutoff 0), norename 2 (largest
      byte 64: 4 of 30 each); the child with RF_HEAD6=0 stays green.
"""
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
POOL = np.concatenate([ALNUM, np.arange(33, 41, dtype=np.uint8)])  # the alphabets are its first D entries
DS = (62, 63, 64, 65)
N = 64 * 40 + 17  # 40 tiles and a partial one
PLANT_EVERY = 200  # a near-duplicate of the query every so many candidates
RARE_AT = (3, 12)  # where the base query holds the rarest symbol
CHUNK = 16  # kChunk
U64MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
NONE32 = np.uint32(0xFFFFFFFF)
NORENAME_TOPS = (62, 63, 64)
RF_ERR_HIP = 2  # rapidfuzz_rs_amd._native.RF_ERR_HIP


# ---------------------------------------------------------------------------------------------- what must exist, from D (or the largest byte) and the length alone
def expect_data6(max_code, length):
    """single-length corpus: whole chunks take any 64 codes, a partial last chunk is filled with code 63, which must then be free"""
    return int(max_code < (64 if length % CHUNK == 0 else 63))


def expect_data6_bucketed(max_code, f64):
    return int(max_code < 64 and not f64)


def expect_heads6(max_code):
    return int(max_code < 64)


# ---------------------------------------------------------------------------------------------- inputs (no GPU)
def alphabet(D):
    return POOL[:D].copy()


def base_query(D, seed):
    """64 of the D - 1 common symbols, the rarest one at RARE_AT; the queries of 20 and 40 symbols are its prefixes"""
    q = POOL[np.random.default_rng(seed).integers(0, D - 1, size=64)]
    q[list(RARE_AT)] = POOL[D - 1]
    return q


def _substitute(rng, row, count, symbols, keep):
    """`count` substitutions at positions outside `keep`"""
    free = [int(p) for p in rng.permutation(len(row)) if int(p) not in keep][:count]
    row[free] = symbols[rng.integers(0, len(symbols), size=len(free))]


def payload_row(rng, q, L, j, symbols, rare):
    """planted row j of the payload corpora: the query cut or continued to L symbols with 0..3 substitutions; every third one keeps the rarest symbol where the
    query has it, the others hold a common symbol there (and every fifth of those is rotated by one)"""
    row = np.resize(q, L).copy()
    at_rare = set(np.nonzero(row == rare)[0].tolist())
    if j % 3 == 0:
        _substitute(rng, row, j // 3 % 4, symbols, at_rare)
    else:
        row[row == rare] = symbols[j % 7]
        _substitute(rng, row, j % 4, symbols, set())
        if j % 5 == 4:
            row = np.roll(row, 1)
    return row


def head_row(rng, q, L, j, symbols, rare):
    """planted row j of the head-plane corpora (L >= 16): 0..3 edits inside the first 8 symbols, on and around the rarest symbol at position 3, and every second
    round of the eight kinds one substitution behind the head"""
    row = np.resize(q, L).copy()
    x, y = symbols[(j * 5 + 1) % len(symbols)], symbols[(j * 7 + 2) % len(symbols)]
    kind = j % 8
    if kind == 1:  # the rarest symbol replaced
        row[3] = x
    elif kind == 2:  # a common one replaced by the rarest
        row[5] = rare
    elif kind == 3:  # the rarest transposed with its neighbour
        row[[3, 4]] = row[[4, 3]]
    elif kind == 4:  # a deletion at the front: the rarest moves to position 2
        row = np.concatenate([row[1:], [x]])
    elif kind == 5:  # the rarest inserted at the front
        row = np.concatenate([[rare], row[:-1]])
    elif kind == 6:  # two edits, one of them on the rarest
        row[3], row[6] = x, y
    elif kind == 7:  # three edits
        row[2], row[3], row[7] = rare, x, y
    if j // 8 % 2:
        row[16 + j % (L - 16)] = y
    return row.astype(np.uint8)


def _check_counts(data, D):
    """the corpus holds exactly the first D symbols of POOL and the D-th is strictly the rarest"""
    hist = np.bincount(data, minlength=256)
    assert np.count_nonzero(hist) == D and (hist[POOL[:D]] > 0).all(), np.count_nonzero(hist)
    assert hist[POOL[D - 1]] < hist[POOL[:D - 1]].min(), (hist[POOL[D - 1]], hist[POOL[:D - 1]].min())


def rows_corpus(D, L, n=N, seed=0, heads=False):
    """uint8 [n, L] over exactly D distinct symbols, and the base query"""
    rng = np.random.default_rng(1000 * D + 10 * L + seed)
    symbols, rare = POOL[:D - 1], POOL[D - 1]
    q = base_query(D, 77 * D + seed)
    rows = symbols[rng.integers(0, D - 1, size=(n, L))]
    for i in range(D):  # every symbol at least once (rows 1 .. D: no planted row is among them)
        rows[1 + i, i % L] = POOL[i]
    for j, r in enumerate(range(PLANT_EVERY // 2, n, PLANT_EVERY)):
        rows[r] = (head_row if heads else payload_row)(rng, q, L, j, symbols, rare)
    rows = np.ascontiguousarray(rows)
    _check_counts(rows.reshape(-1), D)
    return rows, q


def bucketed_corpus(D, n=N, seed=0):
    """(data, offsets) with lengths 0..80 -- five lengths often enough for whole tiles of their own, the rest in mixed tiles -- and the base query"""
    rng = np.random.default_rng(5000 * D + seed)
    symbols, rare = POOL[:D - 1], POOL[D - 1]
    q = base_query(D, 77 * D + seed)
    lens = rng.integers(0, 81, size=n)
    often = rng.random(n) < 0.45
    lens[often] = np.array([64, 57, 16, 7, 33])[rng.integers(0, 5, size=int(often.sum()))]
    lens[:2] = 40
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    data = symbols[rng.integers(0, D - 1, size=int(offsets[-1]))]
    data[:D] = POOL[:D]  # every symbol at least once (candidates 0 and 1)
    for j, r in enumerate(range(PLANT_EVERY // 2, n, PLANT_EVERY)):
        ln = int(lens[r])
        if ln:
            data[int(offsets[r]):int(offsets[r + 1])] = payload_row(rng, q, ln, j, symbols, rare)
    _check_counts(data, D)
    return data, offsets, q


def norename_corpus(top, L, n=N):
    """RF_NO_RENAME=1: nine digits and the byte `top`; the base query (L symbols) holds `top` at RARE_AT"""
    rng = np.random.default_rng(100 * top + L)
    symbols = np.arange(48, 57, dtype=np.uint8)
    q = symbols[rng.integers(0, 9, size=L)]
    q[list(RARE_AT)] = top
    rows = symbols[rng.integers(0, 9, size=(n, L))]
    rows[1, 0] = top
    for j, r in enumerate(range(PLANT_EVERY // 2, n, PLANT_EVERY)):
        rows[r] = head_row(rng, q, L, j, symbols, np.uint8(top))
    rows = np.ascontiguousarray(rows)
    assert int(rows.max()) == top and len(np.unique(rows)) == 10
    return rows, q


def uniform_offsets(rows):
    return np.arange(rows.shape[0] + 1, dtype=np.uint64) * np.uint64(rows.shape[1])


def code_bytes(data, offsets):
    """(sigma, the byte stored as code 63, as 64, as 65) of this corpus, from the packer's own host layout"""
    from rapidfuzz_rs_amd.corpus import host_layout

    sigma = host_layout(np.ascontiguousarray(data).reshape(-1), offsets)["sigma"]
    inv = np.empty(256, dtype=np.int64)
    inv[sigma] = np.arange(256)
    assert (sigma[inv] == np.arange(256)).all()
    return sigma, int(inv[63]), int(inv[64]), int(inv[65])


def families(q, b63, b64, b65):
    """{name: query} from the base query cut to the wanted length (>= 20 symbols)"""
    assert len(q) >= 20
    b = q.copy()
    b[1] = b63
    b[-7:] = b63
    c = q.copy()
    c[[2, len(q) - 2]] = b64
    c[7] = b65
    c[[10, len(q) - 1]] = 255
    return {"a": q.copy(), "b": b, "c": c, "d": np.full(len(q), b63, dtype=np.uint8)}


# ---------------------------------------------------------------------------------------------- the checker
failures = 0
trace = None
digest = hashlib.sha256()


def fail(line):
    global failures
    failures += 1
    print("FAIL " + line, flush=True)


def plan_fields(text):
    """the key=value words of every `[rf plan] raw=` line"""
    return [dict(w.split("=", 1) for w in ln.split()[2:] if "=" in w) for ln in text.splitlines() if ln.startswith("[rf plan] raw=")]


def mismatches(got, exp):
    if got.dtype == np.uint32:
        exp = np.where(exp == U64MAX, NONE32, exp.astype(np.uint32))
        return np.nonzero(got != exp)[0], exp
    return np.nonzero(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[0], exp


class Group:
    """the calls on one corpus: values against the oracle, the road of every call from its plan line, and at the end the `[rf accel]` lines of the corpus"""

    def __init__(self, tag):
        self.tag, self.text, self.checks, self.bad = tag, [trace.take()], 0, 0  # (from the packing of the corpus on)

    def call(self, what, fn, exp, **road):
        try:
            got, refused = fn(), None
        except RuntimeError as e:  # a launcher that refuses its arguments before anything runs (launch_stream_asm over a structure it cannot serve) is a failed check:
            if getattr(e, "status", RF_ERR_HIP) == RF_ERR_HIP:  # the leg goes on, and the road of the call is still read below; a HIP error ends the process
                raise
            got, refused = None, str(e)
        text = trace.take()
        self.text.append(text)
        self.checks += 1
        if refused is not None:
            self.bad += 1
            digest.update(refused.encode())
            fail(f"{self.tag} {what}: the call was refused: {refused}")
        else:
            digest.update(np.ascontiguousarray(got).tobytes())
            bad, exp = mismatches(got, exp)
            if len(bad):
                self.bad += 1
                fail(f"{self.tag} {what}: {len(bad)} values differ, at {bad[:4].tolist()} got {got[bad[:4]].tolist()} expected {exp[bad[:4]].tolist()}")
        if road:
            plans = plan_fields(text)
            seen = [{k: pl.get(k) for k in road} for pl in plans]
            if not plans or any(pl[k] != str(v) for pl in seen for k, v in road.items()):
                self.bad += 1
                fail(f"{self.tag} {what}: road {seen} where {road} is due")
        return got

    def listed(self, what, got, exp_full):
        """filter_many by index: (indices, values) against the oracle's Somes"""
        keep = np.nonzero(exp_full != U64MAX)[0]
        self.text.append(trace.take())
        self.checks += 1
        digest.update(np.ascontiguousarray(got[0]).tobytes() + np.ascontiguousarray(got[1]).tobytes())
        if not (np.array_equal(got[0], keep.astype(np.uint64)) and np.array_equal(got[1], exp_full[keep].astype(np.uint32))):
            self.bad += 1
            fail(f"{self.tag} {what}: {len(got[0])} listed, {len(keep)} due; first {got[0][:4].tolist()} {got[1][:4].tolist()} due {keep[:4].tolist()} {exp_full[keep][:4].tolist()}")

    def close(self, payload6=None, heads6=None):
        text = "".join(self.text)
        for name, want in (("6-bit payload", payload6), ("head plane at 6 bits", heads6)):
            if want is not None and (f"[rf accel] {name}" in text) != bool(want):
                self.bad += 1
                fail(f"{self.tag}: `[rf accel] {name}` {'missing' if want else 'printed'}: the structure {'was not' if want else 'was'} built")
        print(f"{self.tag}: {self.checks} checks, {self.bad} bad", flush=True)


def main(leg):
    import torch

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as NV
    from oracle import oracle as o

    global trace
    from multitile_lists_check import Trace

    trace = Trace()
    # the switches that would take a call off the road its plan line names (rf_scan.hip launch_state, rf_api_scan.hip corpus_data6): at their defaults
    assert not [k for k in ("RF_PACK6", "RF_STREAM", "RF_ASM_STREAM", "RF_ASM_CHUNK") if k in os.environ], "run without the A/B switches of the 6-bit scans"
    GPU = {"levenshtein": rf.distance.levenshtein, "indel": rf.distance.indel, "lcs_seq": rf.distance.lcs_seq, "jaro": rf.distance.jaro, "jaro_winkler": rf.distance.jaro_winkler, "osa": rf.distance.osa}
    ORA = {"levenshtein": o.levenshtein, "indel": o.indel, "lcs_seq": o.lcs_seq, "jaro": o.jaro, "jaro_winkler": o.jaro_winkler, "osa": o.osa}
    OPS = {"distance": NV.OP_DISTANCE, "similarity": NV.OP_SIMILARITY, "normalized_distance": NV.OP_NORMALIZED_DISTANCE, "normalized_similarity": NV.OP_NORMALIZED_SIMILARITY}
    # slack 0.9 / 0.55 / 0.75 of the maximum: above the 0.4 from which an LCS scan keeps its streaming loop (plan(), rf_api_scan.hip), so the f64 table serves them
    CUTS = ((NV.OP_NORMALIZED_SIMILARITY, 0.1), (NV.OP_NORMALIZED_SIMILARITY, 0.45), (NV.OP_NORMALIZED_DISTANCE, 0.75))

    def queries(q64, data, offsets, lengths):
        _, b63, b64, b65 = code_bytes(data, offsets)
        return [(f"query {fam}{ln}", bytes(qq)) for ln in lengths for fam, qq in families(q64[:ln], b63, b64, b65).items()]

    def lcs_checks(g, corpus, rows, qs, d6, metrics=("indel", "lcs_seq"), cuts=True, ratio=True):
        """single-length corpus: the four ops, the loose normalized cutoffs and fuzz ratio; data6 = d6 on every call"""
        for qname, q in qs:
            for metric in metrics:
                bc, ob = GPU[metric].BatchComparator(q), ORA[metric].BatchComparator(q)
                for opname, op in OPS.items():
                    g.call(f"{metric} {opname} {qname}", lambda: bc.many(op, corpus), ob.rows(op, rows, nthreads=8), data6=d6)
                for op, cut in CUTS if cuts else ():
                    g.call(f"{metric} op {op} cutoff {cut} {qname}", lambda: bc.many(op, corpus, score_cutoff=cut), ob.rows(op, rows, nthreads=8, score_cutoff=cut), data6=d6)
            if ratio:
                g.call(f"fuzz ratio {qname}", lambda: rf.fuzz.RatioBatchComparator(q).similarity_many(corpus),
                       ORA["lcs_seq"].BatchComparator(q).rows(NV.OP_NORMALIZED_SIMILARITY, rows, nthreads=8), data6=d6)

    def head_checks(g, corpus, rows, qs, metrics, cutoffs, h6):
        for qname, q in qs:
            for metric in metrics:
                bc, ob = GPU[metric].BatchComparator(q), ORA[metric].BatchComparator(q)
                full = ob.rows(NV.OP_DISTANCE, rows, nthreads=8)
                for k in cutoffs:
                    exp = np.where(full <= np.uint64(k), full, U64MAX)
                    g.call(f"{metric} distance<={k} {qname}", lambda: bc.distance_many(corpus, score_cutoff=k), exp, heads8=1, heads6=h6)
                    g.listed(f"{metric} filter_many<={k} {qname}", bc.filter_many(NV.OP_DISTANCE, corpus, capacity=len(rows), order=NV.FILTER_BY_INDEX, score_cutoff=k), exp)

    if leg == "payload":
        assert os.environ.get("RF_PACK6_MIN_TILES") == "1"
        for D in DS:
            for L in (64, 57, 7):
                rows, q64 = rows_corpus(D, L)
                d6 = expect_data6(D - 1, L)
                corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
                g = Group(f"payload D={D} rows of {L} data6={d6}")
                lcs_checks(g, corpus, rows, queries(q64, rows, uniform_offsets(rows), (20, 40)), d6)
                g.close(payload6=d6)
                del corpus

    elif leg == "bucketed":
        assert os.environ.get("RF_PACK6_MIN_TILES") == "1"
        for D in DS:
            data, offsets, q64 = bucketed_corpus(D)
            corpus = rf.Corpus.from_ragged(data, offsets)
            g = Group(f"bucketed D={D} data6={expect_data6_bucketed(D - 1, False)} (u32 ops)")
            for qname, q in queries(q64, data, offsets, (20, 40)):
                for metric in ("indel", "lcs_seq", "levenshtein"):
                    bc, ob = GPU[metric].BatchComparator(q), ORA[metric].BatchComparator(q)
                    for opname, op in OPS.items():
                        d6 = expect_data6_bucketed(D - 1, op >= NV.OP_NORMALIZED_DISTANCE) if metric != "levenshtein" else 0
                        g.call(f"{metric} {opname} {qname}", lambda: bc.many(op, corpus), ob.many(op, data, offsets, nthreads=8), data6=d6)
            g.close(payload6=expect_data6_bucketed(D - 1, False))
            del corpus

    elif leg == "heads":
        assert os.environ.get("RF_HEAD8_MIN") == "1" and os.environ.get("RF_BAND_FILTER") == "1"
        plane6 = os.environ.get("RF_HEAD6") != "0"
        for D in DS:
            for L in (40, 64):
                rows, q64 = rows_corpus(D, L, heads=True)
                h6 = expect_heads6(D - 1) if plane6 else 0
                corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
                g = Group(f"heads D={D} rows of {L} heads6={h6}")
                _, b63, b64, b65 = code_bytes(rows, uniform_offsets(rows))
                qs = [(f"query {fam}{L}", bytes(qq)) for fam, qq in families(q64[:L], b63, b64, b65).items() if fam != "d"]
                one = q64[:L].copy()
                one[6] = b63  # (families b and c are beyond cutoff 3 of every row when their bytes are absent: this one is a single edit inside the head)
                qs.append((f"query a{L} with the code-63 byte at 6", bytes(one)))
                head_checks(g, corpus, rows, qs, ("levenshtein", "osa"), (0, 1, 2, 3), h6)
                g.close(heads6=h6)
                del corpus

    elif leg == "jaro":
        # values only: no trace names the kernel.  Queries of 40 and 64 symbols over rows of 64 keep launch_jaro_word's asm_ok true (the truncated candidate length stays
        # 64: a multiple of 16, <= 64), which is what lets RF_JARO_PRIV=1 reach jaro_word_asm_kernel<true> while max_stored_sym < 64; a query of 20 would not
        for D in (63, 64, 65):
            rows, q64 = rows_corpus(D, 64)
            corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
            g = Group(f"jaro D={D} rows of 64 RF_JARO_PRIV={os.environ.get('RF_JARO_PRIV')}")
            for qname, q in queries(q64, rows, uniform_offsets(rows), (40, 64)):
                for metric in ("jaro", "jaro_winkler"):
                    g.call(f"{metric} similarity {qname}", lambda: GPU[metric].BatchComparator(q).similarity_many(corpus),
                           ORA[metric].BatchComparator(q).rows(NV.OP_SIMILARITY, rows, nthreads=8))
            g.close()
            del corpus

    elif leg == "norename":
        assert os.environ.get("RF_NO_RENAME") == "1" and os.environ.get("RF_PACK6_MIN_TILES") == "1" and os.environ.get("RF_HEAD8_MIN") == "1"
        for top in NORENAME_TOPS:
            for L in (57, 64):
                rows, q = norename_corpus(top, L)
                sigma, b63, b64, b65 = code_bytes(rows, uniform_offsets(rows))
                assert (sigma == np.arange(256)).all() and (b63, b64, b65) == (63, 64, 65)  # the stored code is the byte
                d6, h6 = expect_data6(top, L), expect_heads6(top)
                corpus = rf.Corpus.from_rows(rows)
                g = Group(f"norename largest byte {top} rows of {L} data6={d6} heads6={h6}")
                qs = [(f"query {f}{ln}", bytes(families(q[:ln], 63, 64, 65)[f])) for ln in (20, 40) for f in "bd"]
                assert all(63 in qq for _, qq in qs)
                lcs_checks(g, corpus, rows, qs, d6, metrics=("indel",), ratio=False)
                qh = q.copy()
                if top != 63:
                    qh[6] = 63  # (one substitution against every planted row of a corpus without byte 63: the rows within cutoff 2 have one edit more at the most)
                assert 63 in qh
                head_checks(g, corpus, rows, [("query with byte 63", bytes(qh))], ("levenshtein",), (2,), h6)
                g.close(payload6=d6, heads6=h6)
                del corpus

    elif leg == "saveload":
        assert os.environ.get("RF_PACK6_MIN_TILES") == "1"
        D, L = 63, 57
        rows, q64 = rows_corpus(D, L)
        d6 = expect_data6(D - 1, L)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "edge.rfc")
            rf.Corpus.from_rows(rows).save(path)
            corpus = rf.Corpus.load(path)
            assert len(corpus) == len(rows)
            g = Group(f"saveload D={D} rows of {L} data6={d6}")
            lcs_checks(g, corpus, rows, queries(q64, rows, uniform_offsets(rows), (20, 40)), d6, metrics=("indel",), ratio=False)
            g.close(payload6=d6)
            del corpus
    else:
        raise SystemExit(f"unknown leg {leg!r}")


if __name__ == "__main__":
    assert os.environ.get("RF_TRACE_PLAN") and os.environ.get("RF_PACK_TIMING"), "run with RF_TRACE_PLAN=1 RF_PACK_TIMING=1"
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    t_start = time.time()
    try:
        main(sys.argv[1] if len(sys.argv) > 1 else "payload")
    finally:
        if trace is not None:
            trace.close()  # (a traceback goes to the real stderr)
    print(f"SECONDS {time.time() - t_start:.1f}")
    print("DIGEST", digest.hexdigest())
    print("FAILURES", failures)
    sys.exit(1 if failures else 0)
