"""Run by tests/test_gpu_parity.py::test_list_walking_kernels_many_units_per_wavefront in a subprocess with RF_SCAN_BLOCKS_PER_CU=1 and RF_TRACE_PLAN=1.

The sibling checker (tests/multitile_rowdp_check.py) gives every wavefront of a scan_grid() launch four tiles.  This one does the same for the launches that walk a
LIST of survivors: head_filter_kernel (a wavefront per PAIR of tiles, a look-ahead of two pairs that cycles fully only from the third pair on), lane_list_pack_kernel /
tile_list_pack_kernel (a thread per segment: the 4-at-a-time copy loop and a first_of[] boundary inside a segment need segments of five entries and more),
sparse_lean_kernel (the next dense tile's sources and first chunk are requested while this one runs: `cur = nxt; chunk = chunk_next`, also after an early `dead`
break; the second topk_refresh_bound at the ninth tile a wavefront keeps), early_lean_kernel over a tile list, sparse_words_kernel (second pass of a hinted scan) and
band_sparse_kernel (second pass of the small-band hand-over).  Their grids are CUs x 32 / 16 / 8 by default: a wavefront owns a second unit only when the SURVIVORS
outnumber CUs x 32 x 4 x 64 = 2.1 M on 256 CUs, which no other test reaches.  list_max_grid() (rf_scan.hip) caps those factors by RF_SCAN_BLOCKS_PER_CU, so with the
knob at 1 every such launch has at most W = 4 x CUs wavefronts (band_sparse_kernel: 4 x max(1, band_grid / 2)), and the corpora here are sized from the CU count so
that every wavefront of the launch under test owns at least FLOOR[...] units.  That is asserted BEFORE a value is looked at: from the inputs where it follows from them
(a row that carries the query's first 8 symbols survives any correct first pass: the survivors are at least the rows built that way, counted on the host; the lanes a
hinted scan lists are the rows whose oracle distance exceeds 31), from the `[rf plan]` trace where it does not (band_report's survivor count), and the road taken is
read from the trace too (`[rf road] two-pass:`, `hint lists:`, `filter: lane compaction`).  tests/test_scan_grid.py holds the arithmetic below to the launchers' formulas.

argv[1] is the mode; one line per kernel and shape with n and the units per wavefront; `FAILURES n` last; exit status 0 = all equal.  A mismatch is a value: the mode
runs to its end.  A HIP error raises and ends the process, and so does a precondition that does not hold (the mode fails, it does not skip).

  lanes  RF_HEAD8_MIN=1 RF_BAND_FILTER=1: head_filter_kernel<..., kLanes>, lane_list_pack_kernel, sparse_lean_kernel for LevState<1> (query 64 x rows 64), Lev32State
         (30 x 32) and OsaState<1> (64 x 64), cutoffs 3 (the band test) and 5 (the first look runs in the pass).  Shape A: every row carries the query's head, so every
         row survives and its dense tile follows from the inputs: 10 per wavefront, 5 pairs per listing wavefront, 10 entries and more per segment.  The wavefronts whose number is a multiple
         of 4 find a row within the cutoff in every tile they own (their top-k lists reach the second refresh of the bound); the tiles of the others hold, at random,
         1..3 rows within the cutoff or rows that equal the query for 0 / 16 / 32 / 48 symbols and are noise from there on: one walk mixes tiles that die at chunk
         ends 1, 2 and 3 with tiles that live to the end.  Shape B: a row carries the head with probability 1/2, so a dense tile straddles corpus tiles and a
         first_of[] boundary falls inside an entry; 4 per wavefront.  distance_many, a normalized op under an f64 cutoff, filter_many by index and by score with
         capacity = n, the top-16 under cutoff 3 (the normalized op under the cutoff that allows 3 edits: one
         that allows 5 has its first look at column 10, beyond the head plane).  RF_HEAD6=0 in a second child: the 8-byte plane's load_pair.
  tiles  ... RF_LANE_COMPACT=0: head_filter_kernel (tiles form), tile_list_pack_kernel, early_lean_kernel over the list.  Shape A, distance_many and the top-16.
  runs   a corpus of lengths 63 and 64, each one length run (run_orig, kPad, the pre-filled out) of 4 W + 1 exact tiles whose rows all carry the head; distance_many,
         filter_many, and RF_FLAG_SLOT_ORDER mapped back through slot_index() walk the runs; topk (which keeps a bucketed corpus on the general cutoff kernels) is
         compared with them.
  hint   RF_HINT_SAMPLE_MIN_TILES=1: band_list_kernel, lane_list_pack_kernel, sparse_words_kernel for queries of 100 (2 words) and 300 (5 words) symbols, rows 4 longer /
         shorter, 75 % of them near the query (drawn from a pool of tests/test_gpu_filter._band_rows(..., kinds=6) rows); score_hint 8 / 31 x score_cutoff None / 40 /
         200, two calls each, against the un-hinted oracle.
  band   RF_BAND_DEFER_ADAPT=0 (every launch hands over, whatever the last one reported): band_defer_kernel, lane_list_pack_kernel, band_sparse_kernel, query 256 x
         rows 256, half of them near the query, cutoffs 8 and 31.  The survivors of a call are printed by the NEXT call on the stream (the host reads band_report then).
         RF_ASM_BAND=0 in a second child.

A corpus has 64 x (units x W + 1) - 27 candidates: not a multiple of 64, and an ODD number of tiles (units x W is even), so that the last pair's second half is the head
plane's pad row.

The packed list is NOT in index order once a listing wavefront owns several pairs: wavefront g takes the pairs g, g + G, ..., so a candidate's dense tile follows
from list_position() below, not from its index.  (An earlier version of this file took dense tile j for corpus tile j; its shape A top-16 then had its winners in
most wavefronts' FIRST units and stayed green under the first planted error below.)

Planted errors tried on an MI355X (not committed), lines with mismatches / lines: sparse_lean_kernel keeping `chunk` for the next dense tile 36 / 36 in lanes (every
top-16 line loses all 16 winners); head_filter_kernel's `packed = ahead2` 24 / 36; lane_list_pack_kernel's 4-entry loop without the last `run += c` 30 / 36;
sparse_words_kernel's st.init() before the loop only 8 / 12 in hint (the cases under score_cutoff=40 stay green).

Seconds per mode, measured once on an MI355X (256 CUs, W = 1024; 655 397 candidates in shape A): MEASURED_SECONDS below; the timeouts of the test are about three
times these, and at least 60 s.
"""
import os
import sys
import tempfile
import time

import numpy as np

MEASURED_SECONDS = {"lanes": 4, "lanes-head8": 4, "tiles": 3, "runs": 3, "hint": 3, "band": 3, "band-compiled": 3}  # whole child process, wall clock
FLOOR = {"lanes A": 10, "lanes A pairs": 5, "lanes B": 4, "tiles": 4, "runs": 4, "hint": 4, "band": 4}  # units per wavefront; "tiles" runs shape A and prints 10
WAVES = 4  # kWavesPerBlock
DEFAULT_PER_CU = 32  # RF_SCAN_BLOCKS_PER_CU unset


# ---------------------------------------------------------------------------------------------- the grid arithmetic (no GPU; tests/test_scan_grid.py reads these)
def list_max_grid(cus, factor, knob=None):
    """list_max_grid() of rf_scan.hip: CUs x min(the launch's own factor, RF_SCAN_BLOCKS_PER_CU)"""
    return cus * min(factor, DEFAULT_PER_CU if knob is None else knob)


def sparse_lean_grid(tiles, cus, knob=None, small=False):
    """launch_sparse_lean (rf_sparse.hip); `small`: with top-k lists or over a length run"""
    return max(1, min(list_max_grid(cus, 8 if small else 32, knob), (tiles + WAVES - 1) // WAVES))


def sparse_words_grid(tiles, cus, knob=None):
    """launch_sparse_words (rf_sparse.hip)"""
    return max(1, min(list_max_grid(cus, 16, knob), (tiles + WAVES - 1) // WAVES))


def head_filter_grid(tiles, cus, knob=None):
    """head_list_layout (rf_scan.hip): workgroups of the listing pass, a wavefront per pair of tiles"""
    pairs = (tiles + 1) // 2
    return min((pairs + WAVES - 1) // WAVES, min(list_max_grid(cus, 16, knob), 4096))


def early_list_grid(cus, knob=None):
    """early_lean_kernel over a tile list (launch_early, rf_scan.hip): a fixed grid"""
    return list_max_grid(cus, 8, knob)


def band_grid(tiles, cus, knob=None):
    """band_grid_of (rf_band.hip): half of scan_max_grid() at most"""
    most = cus * (DEFAULT_PER_CU if knob is None else knob)
    return max(1, min(min((tiles + WAVES - 1) // WAVES, most), (most + 1) // 2))


def band_sparse_grid(tiles, cus, knob=None):
    """band_sparse_kernel (launch_band): half the first pass' grid"""
    return max(1, band_grid(tiles, cus, knob) // 2)


def capped_waves(cus):
    """W: the wavefronts of a list-walking launch at RF_SCAN_BLOCKS_PER_CU=1, when its list is long enough to fill the grid"""
    return WAVES * cus


def units_per_wavefront(units, grid):
    """the fewest units a wavefront of `grid` workgroups owns: wavefront w takes units w, w + stride, ..."""
    return units // (grid * WAVES)


def list_position(tiles, listing_waves):
    """where the listing pass leaves each corpus tile in the packed list: wavefront g of G takes the pairs g, g + G, g + 2 G, ... (head_filter_kernel), its segment
    holds their tiles in that order, and the pack kernels join the segments in order.  With more than one pair per wavefront the list is NOT in index order."""
    pair = np.arange((tiles + 1) // 2)
    by_list = np.lexsort((pair // listing_waves, pair % listing_waves))  # the pairs in list order: by segment, then by round
    order = np.stack([2 * by_list, 2 * by_list + 1], axis=1).reshape(-1)
    order = order[order < tiles]
    pos = np.empty(tiles, dtype=np.int64)
    pos[order] = np.arange(tiles)
    return pos


def survivors_in_front(per_tile, listing_waves):
    """per corpus tile: how many of the rows counted in `per_tile` the list holds in front of that tile's own"""
    pos = list_position(len(per_tile), listing_waves)
    in_order = np.empty(len(per_tile), dtype=np.int64)
    in_order[pos] = per_tile
    return (np.cumsum(in_order) - in_order)[pos]


def tiles_for(per_wave, waves, extra=0):
    """tiles of a corpus that gives each of `waves` wavefronts `per_wave` units: an odd count"""
    return (per_wave * waves + extra) | 1


def band_tiles(cus):
    """tiles of the band mode's corpus: 12 per wavefront of band_sparse_kernel's grid, of which somewhat under half of the lanes are handed over"""
    return tiles_for(12, WAVES * max(1, ((cus + 1) // 2) // 2))


def candidates_of(tiles):
    return 64 * tiles - 27


def derived_shapes(cus):
    """(what, units, grid at the knob = 1, floor) for every corpus this checker sizes from the CU count alone"""
    W = capped_waves(cus)
    a, b4 = tiles_for(10, W), tiles_for(4, W)
    bw = WAVES * band_sparse_grid(band_tiles(cus), cus, 1)
    # what the data-sized lists are EXPECTED to hold, five standard deviations of the draw below the mean: half of shape B's rows carry the head, a quarter of the
    # hint corpus' rows are random (the checker counts the real figures and asserts them)
    nb, nh = candidates_of(tiles_for(8, W, 65)), candidates_of(tiles_for(17, W, 65))
    b_dense = int(nb / 2 - 5 * (nb * 0.25) ** 0.5) // 64
    h_dense = int(nh / 4 - 5 * (nh * 0.1875) ** 0.5) // 64
    return [
        ("lanes A dense tiles", a, sparse_lean_grid(a, cus, 1), FLOOR["lanes A"]),
        ("lanes A dense tiles, top-k", a, sparse_lean_grid(a, cus, 1, small=True), FLOOR["lanes A"]),
        ("lanes A pairs", (a + 1) // 2, head_filter_grid(a, cus, 1), FLOOR["lanes A pairs"]),
        ("lanes B dense tiles", b_dense, sparse_lean_grid(tiles_for(8, W, 65), cus, 1), FLOOR["lanes B"]),
        ("tiles listed", a, early_list_grid(cus, 1), FLOOR["tiles"]),
        ("runs dense tiles", b4, sparse_lean_grid(b4, cus, 1, small=True), FLOOR["runs"]),
        ("runs pairs", (b4 + 1) // 2, head_filter_grid(b4, cus, 1), FLOOR["runs"] // 2),
        ("hint dense tiles", h_dense, sparse_words_grid(tiles_for(17, W, 65), cus, 1), FLOOR["hint"]),
        ("band dense tiles", 4 * bw, band_sparse_grid(band_tiles(cus), cus, 1), FLOOR["band"]),
    ]


# ---------------------------------------------------------------------------------------------- the checker
failures = 0
trace = None
ALNUM = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
OTHER = np.uint8(126)  # a symbol no row and no query holds


class Trace:
    """this process' stderr (the library's `[rf plan]` lines) through a file, so that the checker reads what its own calls printed; passed on to the real stderr"""

    def __init__(self):
        sys.stderr.flush()
        self.real = os.dup(2)
        self.file = tempfile.TemporaryFile()
        os.dup2(self.file.fileno(), 2)
        self.at = 0

    def take(self):
        sys.stderr.flush()
        self.file.seek(self.at)
        text = self.file.read()
        self.at += len(text)
        os.write(self.real, text)
        return text.decode("utf-8", "replace")

    def close(self):
        self.take()
        os.dup2(self.real, 2)


def report(tag, n, units, floor, bad, extra=""):
    global failures
    assert units >= floor, (tag, n, units, floor)  # the condition of this file, before any value is looked at
    print(f"{tag}: n={n} units/wavefront>={units}{extra} {'ok' if not bad else bad}", flush=True)
    failures += len(bad)


def near_row(rng, q, L, kind, lo, subs=None):
    """the query resized to L symbols after 0..3 edits at positions >= lo (the kinds of tests/test_gpu_filter._prefix_corpus); `subs`: that many substitutions"""
    base = np.resize(q, L + 4)
    if kind == 0:
        return base[:L].copy()
    if kind == 1:  # substitutions (inside the part of the row that is the query: each costs exactly one edit)
        row = base[:L].copy()
        row[rng.choice(np.arange(lo, min(L, len(q))), size=int(rng.integers(1, 4)) if subs is None else subs, replace=False)] = OTHER
        return row
    d = int(rng.integers(1, 3))
    if kind == 2:  # d deletions inside the first 12 symbols
        keep = np.ones(L + 4, dtype=bool)
        keep[rng.choice(np.arange(lo, 12), size=d, replace=False)] = False
        return base[keep][:L].copy()
    if kind == 3:  # d insertions inside the first 12 symbols
        row = base.copy()
        for p in sorted(rng.choice(np.arange(lo, 12), size=d, replace=False)):
            row = np.concatenate([row[:p], [OTHER], row[p:]])
        return row[:L].copy()
    row = base[:L].copy()  # a transposition behind the head and one at the end
    row[[9, 10]] = row[[10, 9]]
    row[[L - 2, L - 1]] = row[[L - 1, L - 2]]
    return row


def off_best_row(rng, q, L, lo, first):
    """a near row that is NOT at the corpus' smallest distance b = |L - len(q)| (the unedited row's): substitutions -- b + 1 .. 3 edits for the `first` row of a tile,
    which must stay within cutoff 3 -- or, where b = 0 (any edit costs at least one), the other kinds"""
    b = abs(L - len(q))
    if first or b:
        return near_row(rng, q, L, 1, lo, subs=int(rng.integers(1, 4 - b)) if first else None)
    return near_row(rng, q, L, int(rng.integers(1, 5)), lo)


def shape_a(q, L, tiles, W, seed, late=8, G=None):
    """every row carries the query's first 8 symbols, so every row survives the first pass and a row's DENSE tile follows from the inputs: the rows the list holds
    in front of it (list_position(): G listing wavefronts), by 64.  Wavefront w of the second pass owns the dense tiles w, w + W, ...; see the head of the file.
    Rows at the smallest distance of the corpus sit only in corpus tiles whose rows all land in dense tiles >= late x W -- a wavefront's units late + 1 and later --
    so that the best candidates of a top-k come from units behind a wavefront's first ones (and, at late = 8 in the wavefronts that keep every tile, from behind the
    second refresh of the bound)"""
    rng = np.random.default_rng(seed)
    n = candidates_of(tiles)
    rows = ALNUM[rng.integers(0, 62, size=(n, L))]
    rows[:, :8] = q[:8]
    in_tile = np.minimum(64, n - 64 * np.arange(tiles))
    in_front = survivors_in_front(in_tile, W if G is None else G)
    dense_lo, dense_hi = in_front // 64, (in_front + in_tile - 1) // 64  # the dense tiles of each corpus tile's first and last row
    first_owned, last_owned = dense_lo % W % 4 == 0, dense_hi % W % 4 == 0  # (by a wavefront whose number is a multiple of 4: that row is planted)
    alive = (rng.random(tiles) < 0.35) | first_owned | last_owned
    heads = [h for h in (0, 16, 32, 48) if h < L]
    for t in range(tiles):
        last = min(64, n - 64 * t)
        lanes = rng.choice(last, size=int(rng.integers(1, 4)), replace=False)
        if first_owned[t]:
            lanes = np.concatenate([[0], lanes[lanes != 0]])
        elif last_owned[t]:
            lanes = np.concatenate([[last - 1], lanes[lanes != last - 1]])
        for j, lane in enumerate(lanes):
            if alive[t] and dense_lo[t] >= late * W:  # (the first one unedited: the tile lives to the end under every cutoff here)
                rows[64 * t + lane] = near_row(rng, q, L, int(rng.integers(0, 5)) if j else 0, 8)
            elif alive[t]:  # (the first one within cutoff 3, none at the smallest distance)
                rows[64 * t + lane] = off_best_row(rng, q, L, 8, j == 0)
            else:
                h = heads[int(rng.integers(0, len(heads)))]
                rows[64 * t + lane, :h] = np.resize(q, L)[:h]
    return np.ascontiguousarray(rows)


def shape_b(q, L, tiles, W, seed, G):
    """a row carries the head with probability 1/2; near rows (edits in the head too) and head-then-noise rows anywhere -- rows at the smallest distance of the corpus
    only where the head-carriers that the list holds in front of them fill W dense tiles and 128 more (the planted rows move a few carriers; main() counts again)"""
    rng = np.random.default_rng(seed)
    n = candidates_of(tiles)
    rows = ALNUM[rng.integers(0, 62, size=(n, L))]
    carry = rng.random(n) < 0.5
    rows[carry, :8] = q[:8]
    late = dense_lower_bound(carry, tiles, G) >= W + 128
    picks = rng.choice(n, size=min(6000, n // 4), replace=False)
    for j, i in enumerate(picks):
        if j % 2:
            rows[i] = near_row(rng, q, L, j // 2 % 5, 0) if late[i] else off_best_row(rng, q, L, 0, j % 4 == 1)
        else:
            h = (16, 32, 48)[j // 2 % 3]
            if h < L:
                rows[i, :h] = np.resize(q, L)[:h]
    return np.ascontiguousarray(rows)


def dense_lower_bound(has, tiles, G):
    """per candidate: the dense tile it lands in at least -- the rows marked in `has` (which any correct first pass lists) that the list holds in front of it, by 64;
    exact where every row is marked"""
    padded = np.zeros(tiles * 64, dtype=np.int64)
    padded[:len(has)] = has
    per_tile = padded.reshape(tiles, 64)
    inside = np.cumsum(per_tile, axis=1) - per_tile
    return ((survivors_in_front(per_tile.sum(axis=1), G)[:, None] + inside).reshape(-1)[:len(has)]) // 64


def carriers(rows, q):
    """the rows that any correct first pass lists: their first 8 symbols are the query's"""
    return int(np.count_nonzero((rows[:, :8] == q[:8]).all(axis=1)))


STATES = [("LevState<1>", "levenshtein", 64, 64), ("Lev32State", "levenshtein", 30, 32), ("OsaState<1>", "osa", 64, 64)]


def main(mode):
    global failures
    import torch

    import rapidfuzz_rs_amd as rf
    from rapidfuzz_rs_amd import _native as N
    from rapidfuzz_rs_amd.utils import synth

    import test_gpu_filter as TF

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W = capped_waves(cus)
    print(f"mode {mode}: {cus} CUs, RF_SCAN_BLOCKS_PER_CU=1: list-walking launches have at most {W} wavefronts", flush=True)
    global trace
    trace = Trace()
    U64MAX = TF.U64MAX

    def under(full, k):
        return np.where(full <= np.uint64(k), full, U64MAX)

    def mismatch(what, got, exp):
        miss = TF._same(got, exp)
        return [(what, len(miss), miss[:4].tolist(), got[miss[:4]].tolist(), np.asarray(exp)[miss[:4]].tolist())] if len(miss) else []

    def topk_mismatch(bc, corpus, full, k, cutoff, dense_of=None, from_dense=0):
        """`dense_of`: a lower bound of the dense tile each candidate lands in; every expected winner must sit in dense tile `from_dense` or later (asserted first)"""
        order = np.lexsort((np.arange(len(full)), full))
        want = [(int(full[j]), int(j)) for j in order[:k] if full[j] <= cutoff]
        if dense_of is not None:
            assert len(want) == k and min(int(dense_of[j]) for _, j in want) >= from_dense, (from_dense, [(v, j, int(dense_of[j])) for v, j in want])
        s, i = bc.topk(corpus, k, score_cutoff=cutoff)
        got = list(zip(s.tolist(), i.tolist()))
        return [] if got == want else [(f"topk{k} <= {cutoff}", sum(a != b for a, b in zip(got, want)) + abs(len(got) - len(want)), got[:3], want[:3])]

    def filter_mismatch(bc, corpus, exp, k):
        idx_e, val_e = TF._some(exp)
        bad = []
        idx, val = bc.filter_many(N.OP_DISTANCE, corpus, capacity=len(exp), order=N.FILTER_BY_INDEX, score_cutoff=k)
        if not (bc.last_filter_count == len(idx_e) and np.array_equal(idx, idx_e) and np.array_equal(val, val_e)):
            bad.append((f"filter by index <= {k}", abs(int(bc.last_filter_count) - len(idx_e)) + int(np.count_nonzero(idx[:len(idx_e)] != idx_e[:len(idx)])), len(idx), len(idx_e)))
        idx, val = bc.filter_many(N.OP_DISTANCE, corpus, capacity=len(exp), order=N.FILTER_BY_SCORE, score_cutoff=k)
        want = np.lexsort((idx_e, val_e))
        if not (np.array_equal(idx, idx_e[want]) and np.array_equal(val, val_e[want])):
            bad.append((f"filter by score <= {k}", abs(len(idx) - len(idx_e)) + int(np.count_nonzero(idx[:len(idx_e)] != idx_e[want][:len(idx)])), len(idx), len(idx_e)))
        return bad

    def road_taken(text, form, tiles, calls, **more):
        """every one of `calls` launches took the two-pass road over `tiles` tiles with W listing wavefronts (the `[rf road] two-pass:` lines of rf_scan.hip)"""
        lines = [ln for ln in text.splitlines() if ln.startswith("[rf road] two-pass:")]
        want = f"[rf road] two-pass: {form} list, {tiles} tiles, {WAVES * head_filter_grid(tiles, cus, 1)} listing wavefronts,"
        hits = [ln for ln in lines if ln.startswith(want) and all(f" {k}={v}" in ln for k, v in more.items())]
        assert len(hits) >= calls, (want, more, calls, lines[-6:])

    if mode in ("lanes", "tiles"):
        lanes = mode == "lanes"
        assert (os.environ.get("RF_LANE_COMPACT") == "0") == (not lanes)
        form = "lane" if lanes else "tile"
        for state, metric, qlen, L in STATES:
            q = np.frombuffer(synth.query(qlen, 0x11575 + qlen), dtype=np.uint8)
            bc, ob = TF.GPU[metric].BatchComparator(q.tobytes()), TF.ORA[metric].BatchComparator(q.tobytes())
            for shape in ("A", "B") if lanes else ("A",):
                tiles = tiles_for(10, W) if shape == "A" else tiles_for(8, W, 65)
                G = WAVES * head_filter_grid(tiles, cus, 1)
                rows = shape_a(q, L, tiles, W, seed=qlen + L, G=G) if shape == "A" else shape_b(q, L, tiles, W, 1000 + qlen + L, G)
                n = len(rows)
                assert n == candidates_of(tiles) and n % 64 != 0 and tiles % 2 == 1
                # what the launches under test own, from the inputs: the rows that carry the head survive whatever else does
                have = carriers(rows, q)
                dense = (have + 63) // 64
                if lanes:
                    units = units_per_wavefront(dense, sparse_lean_grid(tiles, cus, 1))
                    units_k = units_per_wavefront(dense, sparse_lean_grid(tiles, cus, 1, small=True))
                else:
                    listed = tiles if shape == "A" else 0  # (shape A: every tile holds a carrier)
                    assert have == n
                    units = units_k = units_per_wavefront(listed, early_list_grid(cus, 1))
                pairs = units_per_wavefront((tiles + 1) // 2, head_filter_grid(tiles, cus, 1))
                floor = FLOOR["lanes " + shape] if lanes else FLOOR["tiles"]
                assert pairs >= (FLOOR["lanes A pairs"] if shape == "A" else floor), (state, shape, pairs)
                if shape == "A":
                    assert have == n and 2 * pairs >= 10  # entries per segment: every tile is listed
                extra = f" pairs/wavefront>={pairs} head-carriers={have}"
                corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
                full = ob.rows(N.OP_DISTANCE, rows, nthreads=8)
                mx = max(qlen, L)
                # the dense tile of every candidate (shape A: exactly, every row survives; shape B: at least, the survivors include the head-carriers), in LIST order
                dense_of = dense_lower_bound((rows[:, :8] == q[:8]).all(axis=1), tiles, G)
                for k in (3, 5):
                    exp = under(full, k)
                    if shape == "A" and k == 3:  # the data is what the head of the file says: most wavefronts walk live and dead tiles
                        live = np.bincount(dense_of[full <= 3], minlength=dense) > 0  # per dense tile
                        assert live[np.arange(dense) % W % 4 == 0].all() and 0.5 < live.mean() < 0.75, live.mean()
                    bad = mismatch(f"distance <= {k}", bc.distance_many(corpus, score_cutoff=k), exp)
                    text = trace.take()
                    road_taken(text, form, tiles, 1, run=0, topk=0)
                    assert ("head_need=0" not in text) == (k == 3), text[-600:]  # cutoff 3: the band test; 5: the look in the pass
                    report(f"{mode} {shape} {state} query={qlen} distance<={k}", n, units, floor, bad, extra)
                    if not lanes:
                        continue
                    if k == 3:  # (an f64 cutoff that allows 3 edits; one that allows 5 moves the first look to column 10, beyond the head plane)
                        ncut = 1.0 - (k + 0.5) / mx
                        got = bc.many(N.OP_NORMALIZED_SIMILARITY, corpus, score_cutoff=ncut)
                        bad = mismatch(f"normalized_similarity >= {ncut:.4f}", got, ob.rows(N.OP_NORMALIZED_SIMILARITY, rows, nthreads=8, score_cutoff=ncut))
                        road_taken(trace.take(), form, tiles, 1, run=0, topk=0)
                        report(f"{mode} {shape} {state} query={qlen} normalized_similarity>={ncut:.4f}", n, units, floor, bad, extra)
                    bad = filter_mismatch(bc, corpus, exp, k)
                    text = trace.take()
                    road_taken(text, form, tiles, 2, run=0, topk=0)
                    assert text.count("[rf plan] filter: lane compaction") >= 2, text[-600:]
                    report(f"{mode} {shape} {state} query={qlen} filter_many<={k}", n, units, floor, bad, extra)
                # the 16 best sit behind every wavefront's first units: shape A in dense tiles 8 W and later, shape B in dense tiles W and later
                from_dense = 8 * W if shape == "A" else W
                bad = topk_mismatch(bc, corpus, full, 16, 3, dense_of, from_dense)
                road_taken(trace.take(), form, tiles, 1, run=0, topk=16)
                report(f"{mode} {shape} {state} query={qlen} topk16<=3 winners-in-dense-tiles>={from_dense}", n, units_k, floor, bad, extra)
                del corpus

    elif mode == "runs":
        q = np.frombuffer(synth.query(64, 0x2075), dtype=np.uint8)
        tiles = tiles_for(4, W)
        assert tiles >= int(os.environ.get("RF_RUN_MIN_TILES", "256")), "a length run this short takes the general kernels"
        rng = np.random.default_rng(6364)
        per_len = {}
        for L in (63, 64):
            r = shape_a(q, L, tiles + 1, W, seed=L, late=2, G=WAVES * head_filter_grid(tiles, cus, 1))  # 64 x tiles + 37 rows: `tiles` exact tiles, 37 rows for the mixed section
            assert len(r) == 64 * tiles + 37 and carriers(r, q) == len(r)
            per_len[L] = r
        lens = np.concatenate([np.full(len(per_len[63]), 63), np.full(len(per_len[64]), 64)])
        which = rng.permutation(len(lens))
        lens = lens[which]
        offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(lens)
        data = np.empty(int(offsets[-1]), dtype=np.uint8)
        taken = {63: 0, 64: 0}
        starts = offsets[:-1].astype(np.int64)
        for L in (63, 64):
            at = starts[lens == L]
            data[(at[:, None] + np.arange(L)[None, :]).reshape(-1)] = per_len[L].reshape(-1)
            taken[L] = len(at)
        n = len(lens)
        corpus = rf.Corpus.from_ragged(data, offsets)
        slot_index = corpus.slot_index()
        real = slot_index != TF.NONE32
        # every row carries the head: each run's exact tiles are its dense tiles
        units = units_per_wavefront(tiles, sparse_lean_grid(tiles, cus, 1, small=True))
        pairs = units_per_wavefront((tiles + 1) // 2, head_filter_grid(tiles, cus, 1))
        extra = f" pairs/wavefront>={pairs} runs of {tiles} exact tiles"
        assert pairs >= FLOOR["runs"] // 2
        for metric in ("levenshtein", "osa"):
            bc, ob = TF.GPU[metric].BatchComparator(q.tobytes()), TF.ORA[metric].BatchComparator(q.tobytes())
            full = ob.many(N.OP_DISTANCE, data, offsets, nthreads=8)
            for k in (3, 5):
                exp = under(full, k)
                bad = mismatch(f"distance <= {k}", bc.distance_many(corpus, score_cutoff=k), exp)
                road_taken(trace.take(), "lane", tiles, 2, run=1, topk=0)
                slots = bc.many(N.OP_DISTANCE, corpus, rf.distance.levenshtein.Args().slot_order(), score_cutoff=k)
                back = np.empty(n, dtype=np.uint32)
                back[slot_index[real]] = slots[real]
                bad += mismatch(f"slot order <= {k}", back, exp)
                road_taken(trace.take(), "lane", tiles, 2, run=1, topk=0)
                bad += filter_mismatch(bc, corpus, exp, k)
                road_taken(trace.take(), "lane", tiles, 4, run=1, topk=0)
                # (the top-k of a bucketed corpus keeps its lists in the general cutoff kernels, rf_api_topk.hip: no run launches, the values all the same)
                bad += topk_mismatch(bc, corpus, full, 16, k)
                report(f"runs {metric} query=64 lengths 63+64 distance_many + slot order + filter_many + topk16 <={k}", n, units, FLOOR["runs"], bad, extra)
        del corpus

    elif mode == "hint":
        tiles = tiles_for(17, W, 65)
        n = candidates_of(tiles)
        for qlen, len2 in ((100, 104), (300, 296)):
            q = synth.query(qlen, 0x4157 + qlen)
            pool = TF._band_rows(16384, len2, q, 0.75, seed=qlen + 750, kinds=6)
            rows = np.ascontiguousarray(pool[np.random.default_rng(qlen).integers(0, len(pool), size=n)])
            corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
            bc, ob = rf.distance.levenshtein.BatchComparator(q), TF.ORA["levenshtein"].BatchComparator(q)
            full = ob.rows(N.OP_DISTANCE, rows, nthreads=8)
            left = int(np.count_nonzero(full > np.uint64(31)))  # what a band pass under max(hint, 31) = 31 answers None: the list
            assert 64 * 4 * W <= left <= 0.3 * n, (left, n)
            units = units_per_wavefront((left + 63) // 64, sparse_words_grid(tiles, cus, 1))
            for hint in (8, 31):
                for cutoff in (None, 40, 200):
                    exp = full if cutoff is None else under(full, cutoff)
                    bad = []
                    for rep in range(2):
                        bad += mismatch(f"call {rep}", bc.many(N.OP_DISTANCE, corpus, score_cutoff=cutoff, score_hint=hint), exp)
                    text = trace.take()
                    assert text.count("[rf plan] hint lists:") == 2, text[-800:]
                    walked = [int(ln.split("walked ")[1].split()[0]) for ln in text.splitlines() if ln.startswith("[rf plan] hint report:")]
                    assert walked and all(v == left for v in walked), (walked, left)  # (the pass' own count: the second call of a case reads what the first left)
                    report(f"hint sparse_words_kernel<{(qlen + 63) // 64}> query={qlen} rows={len2} score_hint={hint} score_cutoff={cutoff}, two calls", n, units, FLOOR["hint"],
                           bad, f" listed={left}")
            del corpus

    elif mode == "band":
        assert os.environ.get("RF_BAND_DEFER_ADAPT") == "0"
        tiles = band_tiles(cus)
        n = candidates_of(tiles)
        grid2 = band_sparse_grid(tiles, cus, 1)
        q = synth.query(256, 0xBA2D + 256)
        rows = TF._band_rows(n, 256, q, 0.5, seed=256 + 50)
        corpus = rf.Corpus.from_device_rows(torch.from_numpy(rows).cuda())
        bc, ob = rf.distance.levenshtein.BatchComparator(q), TF.ORA["levenshtein"].BatchComparator(q)

        for k in (8, 31):
            # three calls: the second and the third print what the first and the second handed over (the host reads band_report at the next launch on the stream; each
            # line carries the band_k of the launch it reports, which is the cutoff; the third call's own count is not printed)
            trace.take()
            got = [bc.distance_many(corpus, score_cutoff=k) for _ in range(3)]
            lines = [ln for ln in trace.take().splitlines() if ln.startswith("[rf plan] band report:")][-2:]
            assert len(lines) == 2, lines
            seen = []
            for ln in lines:
                words = ln.split("listed ")[1].split()
                assert int(ln.split("band_k=")[1]) == k, (k, ln)  # the line reports a launch under THIS cutoff
                seen.append((int(words[0]), int(words[2]), int(words[5])))  # entries, survivors, tiles of the launch
            assert seen[0] == seen[1], seen
            entries, survivors, of = seen[0]
            assert of == tiles and survivors >= 64 * 4 * WAVES * grid2, (k, entries, survivors, of, grid2)
            units = units_per_wavefront((survivors + 63) // 64, grid2)
            exp = ob.rows(N.OP_DISTANCE, rows, nthreads=8, score_cutoff=k)
            bad = [m for c in range(3) for m in mismatch(f"distance <= {k}, call {c}", got[c], exp)]
            report(f"band band_sparse_kernel query=256 rows=256 distance<={k} ({WAVES * grid2} wavefronts)", n, units, FLOOR["band"], bad, f" entries={entries} survivors={survivors}")
        del corpus
    else:
        raise SystemExit(f"unknown mode {mode!r}")


if __name__ == "__main__":
    assert os.environ.get("RF_SCAN_BLOCKS_PER_CU") == "1", "run with RF_SCAN_BLOCKS_PER_CU=1"
    assert os.environ.get("RF_TRACE_PLAN"), "run with RF_TRACE_PLAN=1"
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    t_start = time.time()
    try:
        main(sys.argv[1] if len(sys.argv) > 1 else "lanes")
    finally:
        if trace is not None:
            trace.close()  # (a traceback goes to the real stderr)
    print(f"SECONDS {time.time() - t_start:.1f}")
    print("FAILURES", failures)
    sys.exit(1 if failures else 0)
