"""GPU tests (`-m gpu`) of rf_corpus_take / rf_corpus_take_u32 / rf_corpus_lengths and their Python surface: candidates read back out of the packed corpus.
The truth is the Python list the corpus was packed from, bit for bit.  Round trips of every shape of tests/take_shapes.py through every packer (host, rows,
device rows, file, RF_NO_MIXED_TILES in a child process, the device packer from 65 536 candidates on), both roads (index list, whole corpus); index lists with
repeats, reversal and an index_base; the capacity protocol; `char` corpora without and with overflow symbols (2- and 4-byte raw streams); what the first call
leaves in HBM; four host threads making the first call at once; and the purpose: corpus[i] of a top-k result is at the distance the result says."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

TESTS = os.path.dirname(os.path.abspath(__file__))
if TESTS not in sys.path:  # (a `python -c` child imports this module by name)
    sys.path.insert(0, TESTS)
import take_shapes  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(TESTS)
GPU = 0


def _rows(data, offsets, wide=False):
    o = [int(x) for x in offsets]
    if wide:
        return [data[o[j]:o[j + 1]].tobytes().decode("utf-32-le", "surrogatepass") for j in range(len(o) - 1)]
    return [data[o[j]:o[j + 1]].tobytes() for j in range(len(o) - 1)]


def _round_trip(corpus, cands, what):
    n = len(cands)
    assert len(corpus) == n, what
    assert corpus.to_list() == cands, f"{what}: whole-corpus road"
    data, offsets = corpus.take(np.arange(n))
    assert _rows(data, offsets, corpus.wide) == cands, f"{what}: index road"
    assert corpus.lengths().tolist() == [len(c) for c in cands], f"{what}: lengths()"
    assert corpus.lengths(np.arange(n)[::-1]).tolist() == [len(c) for c in cands][::-1], f"{what}: lengths(indices)"


def _packers(name, cands, tmp_path):
    """(what, corpus) for every way `cands` can reach a packed corpus in this process"""
    import torch

    yield "from_list", rf.Corpus.from_list(cands, device=GPU)
    if name.startswith("len"):  # rows of one length
        rows = np.frombuffer(b"".join(cands), dtype=np.uint8).reshape(len(cands), -1)
        yield "from_rows", rf.Corpus.from_rows(rows, device=GPU)
        yield "from_device_rows", rf.Corpus.from_device_rows(torch.from_numpy(rows.copy()).to(f"cuda:{GPU}"))
        wide_rows = torch.zeros((len(cands), rows.shape[1] + 5), dtype=torch.uint8, device=f"cuda:{GPU}")  # a row stride beyond the length
        wide_rows[:, :rows.shape[1]] = torch.from_numpy(rows.copy()).to(f"cuda:{GPU}")
        yield "from_device_rows (strided)", rf.Corpus.from_device_rows(wide_rows[:, :rows.shape[1]])
    path = str(tmp_path / f"{name}.rfc")
    rf.Corpus.from_list(cands, device=GPU).save(path)
    yield "save -> load", rf.Corpus.load(path, device=GPU)


@pytest.mark.parametrize("name", take_shapes.NAMES)
def test_round_trip_through_every_packer(name, tmp_path):
    cands = take_shapes.shape(name)
    for what, corpus in _packers(name, cands, tmp_path):
        _round_trip(corpus, cands, f"{name} {what}")


def child_round_trips():
    """runs in a child process whose environment holds a pack-time knob"""
    for name in ("ragged", "long", "len17"):
        cands = take_shapes.shape(name)
        _round_trip(rf.Corpus.from_list(cands, device=GPU), cands, f"{name} in the child")
    print("child round trips ok")


def test_round_trip_without_mixed_tiles():
    """RF_NO_MIXED_TILES is read once per process, at pack time: every length padded to whole tiles, so exact tiles end in padding lanes"""
    r = subprocess.run([sys.executable, "-c", "import test_gpu_take as t; t.child_round_trips()"], capture_output=True, text=True, cwd=TESTS,
                       env=dict(os.environ, RF_NO_MIXED_TILES="1", PYTHONPATH=os.pathsep.join([ROOT, TESTS])), timeout=300)
    assert r.returncode == 0 and "child round trips ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def child_slot_map_is_shared_with_the_gather_path():
    """runs in a child process with RF_UNSCATTER_MIN=1000 RF_GATHER_WINDOWS=0: per-candidate results of the 3001-candidate ragged corpus then come home through the
    slot-ordered temporary + gather_results_kernel, which reads a candidate -> slot map of its own kind"""
    from oracle import oracle as o

    cands = take_shapes.shape("ragged")
    n = len(cands)
    data, offsets = rf.corpus.ragged(cands)
    q = bytes(range(0x94 - 15, 0x94 + 15))  # (30 symbols around one the corpus holds often)
    scorer = rf.distance.indel.BatchComparator(q)
    want = o.indel.BatchComparator(q).many(N.OP_DISTANCE, data, offsets).astype(np.uint32)
    idx = np.arange(n)[::-3]
    take_first, scan_first = rf.Corpus.from_list(cands, device=GPU), rf.Corpus.from_list(cands, device=GPU)
    before = scan_first.device_bytes
    assert take_first.device_bytes == before
    # the take builds the map, the scan's gather path adopts it
    assert take_first[idx] == [cands[i] for i in idx]
    assert (scorer.distance_many(take_first) == want).all()
    assert take_first[idx] == [cands[i] for i in idx] and take_first.to_list() == cands
    # the scan builds the map, the take uses it
    assert (scorer.distance_many(scan_first) == want).all()
    after_scan = scan_first.device_bytes
    assert after_scan - before >= 4 * n + 4 * scan_first.slot_count, "the scan did not go through the gather path with a candidate -> slot map"
    assert scan_first[idx] == [cands[i] for i in idx] and scan_first.to_list() == cands
    assert scan_first.device_bytes == after_scan  # no second map
    assert take_first.device_bytes == after_scan  # one map either way
    print("child slot map ok")


def test_the_slot_map_is_shared_with_the_gather_path():
    r = subprocess.run([sys.executable, "-c", "import test_gpu_take as t; t.child_slot_map_is_shared_with_the_gather_path()"], capture_output=True, text=True, cwd=TESTS,
                       env=dict(os.environ, RF_UNSCATTER_MIN="1000", RF_GATHER_WINDOWS="0", PYTHONPATH=os.pathsep.join([ROOT, TESTS])), timeout=300)
    assert r.returncode == 0 and "child slot map ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_the_device_packer_round_trips():
    """from 65 536 candidates on rf_corpus_pack does its per-candidate work on the device (rfgpu.h RF_DEVICE_PACK_MIN)"""
    rng = np.random.default_rng(5)
    n = 65536 + 77
    lengths = rng.integers(0, 41, n)
    data = rng.integers(0, 256, int(lengths.sum())).astype(np.uint8).tobytes()
    ends = np.cumsum(lengths).tolist()
    cands = [data[e - l:e] for l, e in zip(lengths.tolist(), ends)]
    corpus = rf.Corpus.from_list(cands, device=GPU)
    assert corpus.to_list() == cands
    idx = rng.integers(0, n, 2000)
    assert corpus[idx] == [cands[i] for i in idx]


@pytest.fixture(scope="module")
def ragged():
    cands = take_shapes.shape("ragged")
    return cands, rf.Corpus.from_list(cands, device=GPU)


def test_index_lists(ragged):
    import torch

    cands, corpus = ragged
    n = len(cands)
    rng = np.random.default_rng(9)
    data, offsets = corpus.take([])
    assert len(data) == 0 and offsets.tolist() == [0]
    for i in (0, 1, n - 1, cands.index(b"")):
        data, offsets = corpus.take([i])
        assert _rows(data, offsets) == [cands[i]]
    data, offsets = corpus.take(np.arange(n)[::-1])
    assert _rows(data, offsets) == cands[::-1]
    idx = rng.integers(0, n, 1000)
    idx[100:110] = idx[5]  # repeats, for certain
    want = [cands[i] for i in idx]
    data, offsets = corpus.take(idx)
    assert _rows(data, offsets) == want
    base = 10**12
    data_b, offsets_b = corpus.take(idx.astype(np.uint64) + np.uint64(base), index_base=base)
    assert (data_b == data).all() and (offsets_b == offsets).all()
    assert corpus.lengths(idx.astype(np.uint64) + np.uint64(base), index_base=base).tolist() == [len(w) for w in want]
    dev, offsets_d = corpus.take(idx, device_out=True)
    assert dev.is_cuda and dev.dtype == torch.uint8 and (offsets_d == offsets).all()
    assert (dev.cpu().numpy() == data).all()
    with pytest.raises(rf.RfError):
        corpus.take([4, 0, 9], index_base=1)  # (0 lies below the base)


def test_getitem(ragged):
    cands, corpus = ragged
    n = len(cands)
    assert corpus[0] == cands[0] and corpus[n - 1] == cands[n - 1] and corpus[-1] == cands[-1] and corpus[-n] == cands[0]
    assert corpus[np.int64(17)] == cands[17]
    assert corpus[5:40:3] == cands[5:40:3] and corpus[-7:] == cands[-7:] and corpus[10:4] == [] and corpus[::-500] == cands[::-500]
    assert corpus[[3, -3, 3]] == [cands[3], cands[-3], cands[3]]
    assert corpus[np.array([n - 1, 0])] == [cands[-1], cands[0]]
    for bad in (n, -n - 1):
        with pytest.raises(IndexError):
            corpus[bad]
    with pytest.raises(IndexError):
        corpus[[0, n]]


def test_capacity_protocol(ragged):
    cands, corpus = ragged
    n = len(cands)
    L = N.lib()
    idx = np.array([7, 7, 2900, 12, cands.index(b"")], dtype=np.uint64)
    want = [cands[int(i)] for i in idx]
    want_offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    total = int(want_offsets[-1])
    offsets = np.full(len(idx) + 1, 77, dtype=np.uint64)
    assert L.rf_corpus_take(corpus._h, idx.ctypes.data, len(idx), 0, None, 0, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK  # the sizing call
    assert (offsets == want_offsets).all()
    payload = np.full(total + 16, 0xA5, dtype=np.uint8)
    offsets[:] = 77
    assert L.rf_corpus_take(corpus._h, idx.ctypes.data, len(idx), 0, payload.ctypes.data, total - 1, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
    assert (payload == 0xA5).all() and (offsets == want_offsets).all()  # short by exactly one: payload untouched, offsets correct
    offsets[:] = 77
    assert L.rf_corpus_take(corpus._h, idx.ctypes.data, len(idx), 0, payload.ctypes.data, total, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK
    assert payload[:total].tobytes() == b"".join(want) and (payload[total:] == 0xA5).all() and (offsets == want_offsets).all()
    # an index of n: refused on the host, nothing written
    payload[:] = 0xA5
    offsets[:] = 77
    idx[2] = n
    lens = np.full(len(idx), 77, dtype=np.uint32)
    assert L.rf_corpus_take(corpus._h, idx.ctypes.data, len(idx), 0, payload.ctypes.data, len(payload), offsets.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
    assert L.rf_corpus_lengths(corpus._h, idx.ctypes.data, len(idx), 0, lens.ctypes.data, None) == N.RF_ERR_INVALID_ARG
    assert (payload == 0xA5).all() and (offsets == 77).all() and (lens == 77).all()
    # every candidate, with no index list: m must be n
    assert L.rf_corpus_take(corpus._h, None, n - 1, 0, None, 0, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
    assert (offsets == 77).all()


def test_take_u32_of_a_byte_corpus_zero_extends(ragged):
    cands, corpus = ragged
    L = N.lib()
    assert not corpus.wide
    idx = np.array([2, 1500, 3000, 2], dtype=np.uint64)
    offsets = np.zeros(len(idx) + 1, dtype=np.uint64)
    assert L.rf_corpus_take_u32(corpus._h, idx.ctypes.data, len(idx), 0, None, 0, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK
    out = np.full(int(offsets[-1]), 0xA5A5A5A5, dtype=np.uint32)
    assert L.rf_corpus_take_u32(corpus._h, idx.ctypes.data, len(idx), 0, out.ctypes.data, len(out), offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK
    assert out.max(initial=0) <= 0xFF
    assert _rows(out.astype(np.uint8), offsets) == [cands[int(i)] for i in idx]
    n = len(cands)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    assert L.rf_corpus_take_u32(corpus._h, None, n, 0, None, 0, offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK
    out = np.full(int(offsets[-1]), 0xA5A5A5A5, dtype=np.uint32)
    assert L.rf_corpus_take_u32(corpus._h, None, n, 0, out.ctypes.data, len(out), offsets.ctypes.data, N.MEM_HOST, None) == N.RF_OK
    assert out.max(initial=0) <= 0xFF and _rows(out.astype(np.uint8), offsets) == cands


def _wide_cases():
    rng = np.random.default_rng(21)

    def strings(symbols, n, weights=None):
        p = None if weights is None else np.asarray(weights, float) / np.sum(weights)
        lengths = rng.integers(0, 50, n)
        lengths[:3] = (0, 49, 16)
        return ["".join(chr(int(s)) for s in rng.choice(symbols, int(l), p=p)) for l in lengths]

    greek_cyrillic = np.concatenate([np.arange(0x391, 0x3CA), np.arange(0x410, 0x450), [0x20, 0x41]])
    bmp400 = np.concatenate([np.arange(0x4E00, 0x4E00 + 396), [0x20, 0x61, 0x3B1, 0xFFFE]])
    skew = 1.0 / np.arange(1, 401)  # frequent symbols get ids of their own, the tail shares the overflow id
    beyond = bmp400.copy()
    beyond[7] = 0x1F600   # above the BMP, frequent: an id of its own, yet the raw stream needs 4 bytes
    beyond[399] = 0xFFFF  # the 2-byte stream's padding value as a symbol, rare: in the overflow class
    beyond[398] = 0x2F800
    beyond_strings = strings(beyond, 700, skew)
    beyond_strings[5] += chr(0xFFFF) + chr(0x2F800) + chr(0xFFFF)  # (for certain, not by the draw)
    return {
        "greek + cyrillic": (strings(greek_cyrillic, 645), 0, None),
        "400 BMP symbols": (strings(bmp400, 700, skew), 1, 2),
        "beyond the BMP": (beyond_strings, 1, 4),
    }


@pytest.mark.parametrize("case", ["greek + cyrillic", "400 BMP symbols", "beyond the BMP"])
def test_char_corpora(case, tmp_path):
    cands, overflow, _raw_elem = _wide_cases()[case]
    packed = rf.Corpus.from_list(cands, device=GPU)
    path = str(tmp_path / "wide.rfc")
    packed.save(path)
    L = N.lib()
    for what, corpus in (("packed", packed), ("loaded", rf.Corpus.load(path, device=GPU))):
        assert corpus.wide, what
        own, shared = corpus.alphabet_size()
        assert (shared > 0) == bool(overflow), (what, own, shared)
        if case == "beyond the BMP":
            assert any(ord(ch) in (0xFFFF, 0x2F800) for c in cands for ch in c) and any(ord(ch) == 0x1F600 for c in cands for ch in c)
        _round_trip(corpus, cands, f"{case} {what}")
        idx = np.array([2, 0, 644, 2, 1], dtype=np.int64)
        assert corpus[idx] == [cands[i] for i in idx] and corpus[-1] == cands[-1] and isinstance(corpus[0], str)
        dev, offsets = corpus.take(idx, device_out=True)
        host, offsets_h = corpus.take(idx)
        assert host.dtype == np.uint32 and dev.element_size() == 4 and (offsets == offsets_h).all()
        assert (dev.view(__import__("torch").uint8).cpu().numpy().view(np.uint32) == host).all()
        # the byte call refuses a wide corpus, with nothing written
        offs = np.full(3, 77, dtype=np.uint64)
        two = np.array([0, 1], dtype=np.uint64)
        assert L.rf_corpus_take(corpus._h, two.ctypes.data, 2, 0, None, 0, offs.ctypes.data, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
        assert (offs == 77).all()


def test_no_candidate_sized_structure_on_a_single_length_corpus(ragged):
    rng = np.random.default_rng(3)
    single = take_shapes.shape("len20")
    corpus = rf.Corpus.from_list(single, device=GPU)
    before = corpus.device_bytes
    idx = rng.integers(0, len(single), 1024)
    assert corpus[idx] == [single[i] for i in idx]
    assert corpus.device_bytes == before
    cands = ragged[0]
    fresh = rf.Corpus.from_list(cands, device=GPU)
    before = fresh.device_bytes
    idx = rng.integers(0, len(cands), 1024)
    assert fresh[idx] == [cands[i] for i in idx]
    first = fresh.device_bytes
    assert 0 < first - before <= 4 * len(cands)  # the candidate -> slot map, and nothing else
    assert fresh[idx[::-1]] == [cands[i] for i in idx[::-1]] and fresh.to_list() == cands
    assert fresh.device_bytes == first


def test_four_host_threads_make_the_first_take_at_once(ragged):
    """the candidate -> slot map is built lazily: whoever comes first builds it, the others must see a complete one or none"""
    import torch

    cands = ragged[0]
    corpus = rf.Corpus.from_list(cands, device=GPU)
    streams = [torch.cuda.Stream(device=GPU) for _ in range(4)]
    gate = threading.Barrier(4)
    results, errors = [None] * 4, []

    def work(t):
        try:
            idx = np.roll(np.arange(len(cands)), 700 * t)
            gate.wait(timeout=60)
            data, offsets = corpus.take(idx, stream=streams[t].cuda_stream)
            results[t] = _rows(data, offsets) == [cands[i] for i in idx]
        except Exception as e:  # noqa: BLE001 - reported below, in the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errors, errors
    assert results == [True] * 4


def test_the_candidates_of_a_topk_are_at_the_distance_it_reports():
    from oracle import oracle as o

    rng = np.random.default_rng(31)
    cands = list(take_shapes.shape("ragged"))
    q = bytes(rng.integers(97, 123, 40).astype(np.uint8))
    for j, i in enumerate(rng.choice(len(cands), 24, replace=False)):  # near-copies: 0..5 edits of the query
        row = bytearray(q)
        for _ in range(j % 6):
            kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(row) - 1))
            if kind == 0:
                row[at] = int(rng.integers(97, 123))
            elif kind == 1:
                del row[at]
            else:
                row.insert(at, int(rng.integers(97, 123)))
        cands[int(i)] = bytes(row)
    corpus = rf.Corpus.from_list(cands, device=GPU)  # (the host copy could be dropped here: everything below reads the packed form)
    scorer = rf.distance.levenshtein.BatchComparator(q)
    score, idx = scorer.topk(corpus, k=16)
    assert len(idx) == 16 and score[0] == 0 and score[-1] <= 5
    for s, i in zip(score, idx):
        assert o.levenshtein.distance(q, corpus[int(i)]) == int(s), int(i)
    base = 5 * 10**9  # a shard's results are handed straight back
    score_b, idx_b = scorer.topk(corpus, k=16, index_base=base)
    data, offsets = corpus.take(idx_b, index_base=base)
    assert _rows(data, offsets) == [cands[int(i)] for i in idx]
