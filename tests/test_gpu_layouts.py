"""GPU parity tests (`-m gpu`) of every corpus LAYOUT the packers can produce, crossed with every result road.  The default layout fills every exact tile of a
length-bucketed corpus and gives each length's leftovers to mixed tiles; under RF_NO_MIXED_TILES (a pack-time knob, recorded in a saved corpus file) every length is
padded to whole tiles, so the last exact tile of each length ends in padding lanes; RF_NO_RENAME changes the stored codes (and with them the head planes and 6-bit
payloads that exist).  Each layout x corpus shape runs many (u32 / f64), RF_FLAG_SLOT_ORDER + rf_corpus_slot_index, rf_filter_* (every order, capacities, device
output, index_base, no cutoff, cutoffs that pass everything), top-k (k up to and beyond n), many_multi and -- for a saved file -- stream_many, every value against the
CPU oracle.  Layouts other than the default are packed in a child process with their environment (the knobs are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N
from rapidfuzz_rs_amd.utils import synth
from oracle import oracle as o

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:  # (a `python -c` child imports this module by name)
    sys.path.insert(0, TESTS)
from test_gpu_filter import GPU, NONE32, ORA, _filter_check, _same  # noqa: E402
from test_gpu_parity import OPS, _check_many  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(TESTS)
CHILD = os.environ.get("RF_TEST_LAYOUT_CHILD") == "1"

# layout -> pack-time environment.  no_mixed_device packs even the 40 k corpus on the device (RF_DEVICE_PACK_MIN=1), no_mixed_host everything on the host;
# no_rename keeps the default packers (host below 65 536 candidates, device above: both appear across the shapes).  no_mixed_file: a child packs and saves under
# RF_NO_MIXED_TILES, this process (no knob set) loads the file.
LAYOUTS = {
    "mixed": {},
    "no_mixed_device": {"RF_NO_MIXED_TILES": "1", "RF_DEVICE_PACK_MIN": "1"},
    "no_mixed_host": {"RF_NO_MIXED_TILES": "1", "RF_DEVICE_PACK_MIN": "0"},
    "no_rename": {"RF_NO_RENAME": "1"},
    "no_mixed_file": {"RF_NO_MIXED_TILES": "1"},
}
NO_MIXED = ("no_mixed_device", "no_mixed_host", "no_mixed_file")
# shape -> run-time environment (long: band runs from 256 tiles of one length on, so that runs end on padded tiles)
SHAPES = {"S": {}, "M": {}, "L": {}, "long": {"RF_BAND_RUN_MIN_TILES": "256"}, "u32": {}}
DIST, SIM, NDIST, NSIM = N.OP_DISTANCE, N.OP_SIMILARITY, N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY
OPNAME = {v: k for k, v in OPS.items()}


def _widen(b):
    """bytes / uint8 -> u32 code points (an injective relabelling: the byte oracle's values hold)"""
    return np.frombuffer(bytes(b), dtype=np.uint8).astype(np.uint32) * 7 + 0x390


def _make(shape):
    """(data, offsets, counts {length: candidates}, query) of a shape.  Every length holds 64 x tiles + r candidates with r in 1..63, so under RF_NO_MIXED_TILES
    every length's last exact tile is partial; ~3 % of the candidates are the query cut / repeated to their length with 0..4 substitutions."""
    rng = np.random.default_rng({"S": 11, "M": 12, "L": 13, "long": 14, "u32": 15}[shape])
    lens, tiles, qlen = {"S": (range(1, 65), (4, 14), 40), "M": (range(20, 41), (280, 320), 30), "L": (range(57, 65), (2100, 2200), 60),
                         "long": (range(250, 263), (256, 270), 256), "u32": (range(1, 31), (1, 3), 20)}[shape]
    counts = {int(ln): 64 * int(rng.integers(tiles[0], tiles[1] + 1)) + int(rng.integers(1, 64)) for ln in lens}
    q = synth.query(qlen, qlen + 3)
    per = np.repeat(np.array(list(counts), dtype=np.int64), list(counts.values()))
    rng.shuffle(per)
    n = len(per)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(per, dtype=np.uint64)
    data = synth.ALNUM[rng.integers(0, 62, size=int(offsets[-1]))]
    qa = np.frombuffer(q, dtype=np.uint8)
    for i in rng.choice(n, size=n * 3 // 100, replace=False):
        a, b = int(offsets[i]), int(offsets[i + 1])
        row = np.resize(qa, b - a)
        e = int(rng.integers(0, 5))
        if e:
            row[rng.integers(0, b - a, size=e)] = synth.ALNUM[rng.integers(0, 62, size=e)]
        data[a:b] = row
    return data, offsets, counts, q


def _pack(shape, data, offsets):
    if shape == "u32":
        return rf.Corpus.from_ragged_u32(_widen(data.tobytes()), offsets)
    return rf.Corpus.from_ragged(data, offsets)


def _save(shape, path):
    """the `python -c` child of the no_mixed_file legs: pack under this process' knobs, save"""
    data, offsets, _counts, _q = _make(shape)
    _pack(shape, data, offsets).save(path)


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype == np.float64 else a == b))


class _Roads:
    """the result roads of one corpus (packed or loaded here) against the oracle over the same bytes"""

    def __init__(self, shape, corpus, data, offsets, q):
        self.shape, self.corpus, self.data, self.offsets, self.q = shape, corpus, data, offsets, q
        self.n = len(offsets) - 1

    def bc(self, metric, q=None):
        q = self.q if q is None else q
        if metric == "ratio":
            return rf.fuzz.RatioBatchComparator(_widen(q) if self.shape == "u32" else q)
        return GPU[metric].BatchComparator(_widen(q) if self.shape == "u32" else q)

    def ob(self, metric, q=None):
        q = self.q if q is None else q
        return o.fuzz.RatioBatchComparator(q) if metric == "ratio" else ORA[metric].BatchComparator(q)

    def expect(self, metric, op, q=None, **kw):
        # (fuzz::ratio's similarity is the oracle's normalized similarity: tests/test_gpu_filter.py test_filter_c1_shape_every_metric)
        return self.ob(metric, q).many(NSIM if metric == "ratio" else op, self.data, self.offsets, nthreads=8, **kw)

    def many(self, metric, op, **kw):
        if self.shape != "u32" and metric != "ratio":
            return _check_many(metric, self.q, self.data, self.offsets, OPNAME[op], corpus=self.corpus, **kw)
        got = self.bc(metric).many(op, self.corpus, **kw)
        bad = _same(got, self.expect(metric, op, **kw))
        assert len(bad) == 0, (self.shape, metric, op, kw, bad[:5])
        return got

    def slots(self, cases):
        """slot_count = 64 x tiles, slot_index a permutation of 0..n padded with kPad, and many(..., slot_order) mapped back through it = the oracle"""
        si = self.corpus.slot_index()
        assert len(si) == self.corpus.slot_count and self.corpus.slot_count % 64 == 0
        real = si != NONE32
        assert int((~real).sum()) == self.corpus.slot_count - self.n
        assert np.array_equal(np.sort(si[real]), np.arange(self.n, dtype=np.uint32))
        for metric, op, kw in cases:
            got = self.bc(metric).many(op, self.corpus, rf.Args().slot_order(), **kw)
            assert len(got) == self.corpus.slot_count
            back = np.empty(self.n, dtype=got.dtype)
            back[si[real]] = got[real]
            bad = _same(back, self.expect(metric, op, **kw))
            assert len(bad) == 0, ("slot order", self.shape, metric, op, kw, bad[:5])
        return si

    def filters(self, cases, pass_all):
        for metric, op, kw in cases:
            _filter_check(self.bc(metric), self.ob(metric), op, self.corpus, self.expect(metric, op, **kw), **kw)
        # no cutoff, or one nothing fails: exactly n pairs, indices 0..n-1 (the padding slots of a RF_NO_MIXED_TILES corpus are not candidates)
        for metric, op, kw in pass_all:
            bc = self.bc(metric)
            idx, val = bc.filter_many(op, self.corpus, **kw)
            assert bc.last_filter_count == self.n and np.array_equal(idx, np.arange(self.n, dtype=np.uint64)), (self.shape, metric, op, kw, bc.last_filter_count, self.n)
            exp = self.expect(metric, op, **kw)
            assert len(_same(val, exp)) == 0, (self.shape, metric, op, kw)
            idx, _ = bc.filter_many(op, self.corpus, capacity=0, **kw)
            assert len(idx) == 0 and bc.last_filter_count == self.n

    def topk(self, ks):
        for metric, op in (("levenshtein", DIST), ("jaro_winkler", SIM)):
            full = self.expect(metric, op)
            order = np.lexsort((np.arange(self.n), full if op == DIST else -full))
            for k in ks:
                s, i = self.bc(metric).topk(self.corpus, k, op=op)
                m = min(k, self.n)
                assert len(i) == len(s) == m and (i < self.n).all(), (self.shape, metric, k, len(i))
                assert np.array_equal(i, order[:m].astype(np.uint64)), (self.shape, metric, k)
                assert np.array_equal(s.astype(np.float64), full[order[:m]].astype(np.float64)), (self.shape, metric, k)

    def multi(self, cases):
        qs = [self.q, self.q[: max(1, len(self.q) // 2)], self.q[::-1]]
        for metric, op, kw in cases:
            bcs = [self.bc(metric, x) for x in qs]
            rows = GPU[metric].BatchComparator.many_multi(bcs, op, self.corpus, **kw)
            assert rows.shape[0] == len(qs) and rows.shape[1] == self.n
            for j, x in enumerate(qs):
                assert _eq(rows[j], bcs[j].many(op, self.corpus, **kw)), (self.shape, metric, op, kw, j)
                assert len(_same(rows[j], self.expect(metric, op, q=x, **kw))) == 0, (self.shape, metric, op, kw, j)

    def stream(self, path, cases):
        seg = {"S": 256 << 10, "u32": 32 << 10}.get(self.shape, 16 << 20)  # several segments per file
        for metric, op, kw in cases:
            bc = self.bc(metric)
            got = bc.stream_many(op, path, self.n, segment_bytes=seg, **kw)
            assert _eq(got, bc.many(op, self.corpus, **kw)), (self.shape, metric, op, kw)
            assert len(_same(got, self.expect(metric, op, **kw))) == 0, (self.shape, metric, op, kw)


def _check_layout(r, counts, no_mixed, si, loaded):
    """the layout is the one the leg claims: under RF_NO_MIXED_TILES one run of ceil(count / 64) tiles per length, ascending, padding at the end of its last tile;
    packed in this process (whose knobs rf_corpus_layout_host follows too), the slot map is the host packer's"""
    if no_mixed:
        pad = np.zeros(r.corpus.slot_count, dtype=bool)
        at = 0
        for ln in sorted(counts):
            t = -(-counts[ln] // 64)
            pad[at + counts[ln]: at + 64 * t] = True
            at += 64 * t
        assert at == r.corpus.slot_count, (at, r.corpus.slot_count)
        assert np.array_equal(si == NONE32, pad)
    if r.shape != "u32" and not loaded:
        lay = rf.host_layout(r.data, r.offsets)
        assert np.array_equal(si, lay["orig"]) and r.corpus.slot_count == 64 * len(lay["tile_len"])
        assert (lay["n_mixed"] == 0) == no_mixed


def _roads(shape, corpus, no_mixed, path=None):
    data, offsets, counts, q = _make(shape)
    r = _Roads(shape, corpus, data, offsets, q)
    assert len(corpus) == r.n
    if shape in ("S", "u32"):
        ql = len(q)
        cuts = {DIST: (2, 40), SIM: (ql - 4, 1), NDIST: (0.1, 1.0), NSIM: (0.9, 0.0)}
        fcuts = {DIST: (0.1, 1.0), SIM: (0.9, 0.0), NDIST: (0.1, 1.0), NSIM: (0.9, 0.0)}
        many = []
        for metric in ("levenshtein", "osa", "indel", "lcs_seq", "jaro", "jaro_winkler"):
            for op in (DIST, SIM, NDIST, NSIM):
                for cut in (None,) + (fcuts if metric.startswith("jaro") else cuts)[op]:
                    if shape == "u32" and metric == "levenshtein" and op == SIM and cut is not None:
                        continue  # quirk Q2 (_check_many knows the rule; the u32 road compares directly)
                    many.append((metric, op, {} if cut is None else {"score_cutoff": cut}))
        many.append(("ratio", SIM, {"score_cutoff": 0.9}))
    elif shape == "long":
        many = [("levenshtein", DIST, {"score_cutoff": 8}), ("levenshtein", DIST, {"score_cutoff": 8}), ("levenshtein", DIST, {"score_cutoff": 2}),
                ("levenshtein", DIST, {"score_cutoff": 31}), ("levenshtein", NSIM, {"score_cutoff": 0.97})]
    else:
        many = [("levenshtein", DIST, {"score_cutoff": 3}), ("osa", DIST, {"score_cutoff": 3}), ("levenshtein", DIST, {}), ("indel", DIST, {}), ("lcs_seq", DIST, {}),
                ("lcs_seq", SIM, {}), ("indel", NSIM, {}), ("jaro_winkler", SIM, {"score_cutoff": 0.8}), ("ratio", SIM, {"score_cutoff": 0.9})]
    for metric, op, kw in many:
        r.many(metric, op, **kw)
    if shape == "long":
        slot_cases = [("levenshtein", DIST, {"score_cutoff": 8})]
        filt = [("levenshtein", DIST, {"score_cutoff": 8}), ("levenshtein", NDIST, {"score_cutoff": 0.03})]
        pass_all = [("levenshtein", DIST, {})]
    else:
        slot_cases = [("levenshtein", DIST, {"score_cutoff": 3}), ("indel", DIST, {}), ("jaro_winkler", SIM, {}), ("lcs_seq", NSIM, {"score_cutoff": 0.5})]
        filt = [("levenshtein", DIST, {"score_cutoff": 3}), ("osa", DIST, {"score_cutoff": 3}), ("indel", DIST, {"score_cutoff": 12}),
                ("jaro_winkler", SIM, {"score_cutoff": 0.8}), ("levenshtein", NSIM, {"score_cutoff": 0.6}), ("ratio", SIM, {"score_cutoff": 0.9})]
        pass_all = [("levenshtein", DIST, {}), ("indel", DIST, {}), ("lcs_seq", SIM, {}), ("levenshtein", NDIST, {"score_cutoff": 1.0}), ("jaro", SIM, {}),
                    ("jaro", SIM, {"score_cutoff": 0.0})]
    si = r.slots(slot_cases)
    _check_layout(r, counts, no_mixed, si, loaded=path is not None)
    r.filters(filt, pass_all)
    r.topk((1, 16, 300) + ((r.n + 5,) if shape in ("S", "u32") else ()))
    if shape != "long":
        r.multi([("indel", DIST, {}), ("levenshtein", DIST, {"score_cutoff": 3}), ("jaro_winkler", SIM, {"score_cutoff": 0.8})])
    if path is not None:
        r.stream(path, [("levenshtein", DIST, {"score_cutoff": 3}), ("indel", DIST, {}), ("jaro_winkler", SIM, {"score_cutoff": 0.8})])


def _child(node, env):
    """one child pytest process on this leg, with its environment; never retried"""
    r = subprocess.run([sys.executable, "-m", "pytest", f"{os.path.abspath(__file__)}::{node}", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, RF_TEST_LAYOUT_CHILD="1", **env), timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-4000:], r.stderr[-2000:])


LEGS = [(layout, shape) for layout in LAYOUTS for shape in SHAPES]


@pytest.mark.parametrize("layout,shape", LEGS, ids=[f"{a}-{b}" for a, b in LEGS])
def test_layout_roads(layout, shape, tmp_path):
    node = f"test_layout_roads[{layout}-{shape}]"
    if layout == "no_mixed_file":
        path = os.environ.get("RF_TEST_LAYOUT_FILE")
        if not CHILD:
            path = str(tmp_path / f"{shape}.rfc")
            code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_layouts as t; t._save(%r, %r)" % (ROOT, TESTS, shape, path)
            s = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **LAYOUTS[layout]), timeout=600)
            assert s.returncode == 0, s.stderr[-3000:]
            if SHAPES[shape]:
                return _child(node, dict(SHAPES[shape], RF_TEST_LAYOUT_FILE=path))
        _roads(shape, rf.Corpus.load(path), True, path=path)
        return
    if not CHILD and (LAYOUTS[layout] or SHAPES[shape]):
        return _child(node, dict(LAYOUTS[layout], **SHAPES[shape]))
    data, offsets, _counts, _q = _make(shape)
    _roads(shape, _pack(shape, data, offsets), layout in NO_MIXED)
