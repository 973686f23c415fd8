"""`char` (u32) corpora packed on the device, and ragged input that already sits in device memory (rf_corpus_pack_device, rf_corpus_pack_u32_device; the device
road of rf_corpus_pack_u32: rf_pack_wide.hip in front of rf_pack_ragged.hip).  The host packer stays the specification: every corpus below is packed by it too
and the two must SAVE to identical files -- header, tiles, slot maps, alphabet section, every payload byte and every raw symbol.

The shapes are the ones at which the new code can go wrong: lengths 0, 1, 15, 16, 17, 31, 32, 33 and 64 around the 16-symbol chunk, three of them with more
than 64 candidates (exact tiles) and the rest with fewer (mixed tiles and their one-length views), one corpus of a single length whose n is no multiple of 64
(the identity layout); offsets that start at 12 345; the last candidate ending exactly at n_elems (a 16-byte load there would leave the caller's buffer);
alphabets of 40, exactly 254, 255 with a count tie at the id boundary, ~3 000 Zipf-distributed BMP symbols (a 2-byte raw stream), the same with 1 % symbols at
or above 0x10000 and one 0xFFFF (a 4-byte raw stream), and runs in which all 64 lanes of many wavefronts count the same symbol."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["a40", "a254_window", "a255_tie", "zipf3000", "zipf3000_astral_window", "same_symbol_runs", "single_length"]


def _lengths(rng, n):
    """16, 32 and 64 take most candidates (exact tiles, and leftovers); every other length stays below 64 candidates (mixed tiles only)"""
    lens = rng.choice(np.array([16, 32, 64]), size=n, p=[0.5, 0.3, 0.2])
    rare = rng.permutation(n)[: 6 * 40].reshape(6, 40)
    for row, ln in zip(rare, [0, 1, 15, 17, 31, 33]):
        lens[row] = ln
    return lens


def _zipf(rng, symbols, size):
    w = 1.0 / np.arange(1, len(symbols) + 1) ** 1.1
    return rng.choice(symbols, size=size, p=w / w.sum()).astype(np.uint32)


def make_case(name):
    """(data uint32, offsets uint64, expected (alphabet, overflow) sizes or None)"""
    rng = np.random.default_rng(CASES.index(name) + 100)
    n = {"a40": 3000, "a254_window": 5000, "a255_tie": 4000, "zipf3000": 20000, "zipf3000_astral_window": 12000, "same_symbol_runs": 9000, "single_length": 3001}[name]
    lens = np.full(n, 17) if name == "single_length" else _lengths(rng, n)
    total = int(lens.sum())
    expect = None
    if name == "a40":
        syms = np.concatenate([np.arange(0x61, 0x61 + 20), np.arange(0x430, 0x430 + 20)]).astype(np.uint32)
        data = rng.choice(syms, size=total).astype(np.uint32)
        data[:40] = syms
        expect = (40, 0)
    elif name == "a254_window":
        syms = (0x4E00 + 7 * np.arange(254)).astype(np.uint32)
        data = _zipf(rng, syms, total)
        data[:254] = syms
        expect = (254, 0)
    elif name == "a255_tie":
        syms = (0x3041 + np.arange(253)).astype(np.uint32)
        data = rng.choice(syms, size=total).astype(np.uint32)  # every one of them thousands of times
        at = rng.permutation(total)[:6]
        data[at[:3]] = 0x9000  # two more symbols, three times each: they tie for rank 253, and the smaller one gets the last id
        data[at[3:]] = 0x8FFF
        expect = (254, 1)
    elif name in ("zipf3000", "zipf3000_astral_window", "single_length"):
        syms = rng.permutation(np.arange(0x4E00, 0x9FA0))[:3000].astype(np.uint32)  # both halves of the BMP table
        data = _zipf(rng, syms, total)
        if name != "zipf3000":
            hi = rng.random(total) < 0.01
            astral = np.concatenate([np.arange(0x10000, 0x10000 + 300), np.arange(0x1F600, 0x1F600 + 300), [0x10FFFF, 0xFFFFFFFE]]).astype(np.uint32)
            data[hi] = _zipf(rng, astral, int(hi.sum()))
            data[total // 2] = 0xFFFF
    else:  # same_symbol_runs: stretches of 4096 equal symbols, so that whole wavefronts of the histogram meet on one counter, in front of a Zipf tail
        syms = rng.permutation(np.arange(0x20, 0xFFF0))[:3000].astype(np.uint32)
        data = _zipf(rng, syms, total)
        for k in range(0, total - 4096, 3 * 4096):
            data[k:k + 4096] = syms[(k // 4096) % 5]
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    if name.endswith("_window"):  # a window into a larger buffer: the offsets start at 12 345, and the last candidate still ends exactly at n_elems
        offsets = offsets + np.uint64(12345)
        data = np.concatenate([data[:12345][::-1], data])  # (the packers count what lies in front of the window too: it holds no symbol of its own)
    assert int(offsets[-1]) == len(data)
    return data, offsets, expect


def as_bytes(data):
    return (data % np.uint32(251)).astype(np.uint8)


def _saved(corpus, path):
    corpus.save(str(path))
    return open(path, "rb").read()


def _same_bytes(a, b, what):
    assert len(a) == len(b), what
    if a != b:
        x, y = np.frombuffer(a, dtype=np.uint8), np.frombuffer(b, dtype=np.uint8)
        bad = np.nonzero(x != y)[0]
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:8]}")


def _device(data, offsets):
    import torch

    wide = data.dtype == np.uint32
    d = torch.from_numpy(data.view(np.int32) if wide else data).cuda()
    o = torch.from_numpy(offsets.view(np.int64)).cuda()
    return d, o


CHILD = r"""
import sys, numpy as np
sys.path.insert(0, sys.argv[1])
import rapidfuzz_rs_amd as rf
work, names = sys.argv[2], sys.argv[3].split(",")
for name in names:
    data, offsets = np.load(f"{work}/{name}.data.npy"), np.load(f"{work}/{name}.offsets.npy")
    print("case", name, file=sys.stderr, flush=True)
    rf.Corpus.from_ragged_u32(data, offsets).save(f"{work}/{name}.{sys.argv[4]}.rfc")
"""


@pytest.fixture(scope="module")
def children(tmp_path_factory):
    """Leg 2, once for all cases: the host entry rf_corpus_pack_u32 in two child processes, RF_DEVICE_PACK_MIN=1 (the device road, with RF_PACK_TIMING=1) and
    =0 (the host packer).  -> (directory, stderr of the device child split per case)"""
    work = tmp_path_factory.mktemp("pack_wide")
    for name in CASES:
        data, offsets, _ = make_case(name)
        np.save(work / f"{name}.data.npy", data)
        np.save(work / f"{name}.offsets.npy", offsets)
    script = work / "child.py"
    script.write_text(CHILD)
    logs = {}
    for tag, env in (("dev", {"RF_DEVICE_PACK_MIN": "1", "RF_PACK_TIMING": "1"}), ("host", {"RF_DEVICE_PACK_MIN": "0"})):
        e = {k: v for k, v in os.environ.items() if k not in ("RF_PACK_TIMING", "RF_DEVICE_PACK_MIN")}
        r = subprocess.run([sys.executable, str(script), ROOT, str(work), ",".join(CASES), tag], capture_output=True, text=True, cwd=ROOT, env=dict(e, **env), timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        logs[tag] = r.stderr
    per_case = {}
    for chunk in logs["dev"].split("case ")[1:]:
        per_case[chunk.split("\n", 1)[0].strip()] = chunk
    assert "device:" not in logs["host"]
    return work, per_case


@pytest.fixture(scope="module")
def packed():
    """per case: the input, the host-packed corpus (n < 65 536: rf_corpus_pack_u32 is the host packer here) and the corpus of the device entry point"""
    cache = {}

    def get(name):
        if name not in cache:
            data, offsets, expect = make_case(name)
            host = rf.Corpus.from_ragged_u32(data, offsets)
            dev = rf.Corpus.from_device_ragged(*_device(data, offsets))
            cache[name] = (data, offsets, expect, host, dev)
        return cache[name]

    return get


@pytest.mark.parametrize("name", CASES)
def test_device_entry_points_save_what_the_host_packer_saves(name, packed, tmp_path):
    data, offsets, expect, host, dev = packed(name)
    _same_bytes(_saved(dev, tmp_path / "dev.rfc"), _saved(host, tmp_path / "host.rfc"), f"{name}: rf_corpus_pack_u32_device")
    assert dev.wide and dev.device_bytes == host.device_bytes and len(dev) == len(offsets) - 1
    if expect is not None:
        assert host.alphabet_size() == expect
    if name.startswith("zipf3000") or name in ("same_symbol_runs", "single_length"):
        assert host.alphabet_size()[1] > 2000  # a raw stream is there
    # the same lengths over bytes: rf_corpus_pack_device against rf_corpus_pack
    b = as_bytes(data)
    hb = rf.Corpus.from_ragged(b, offsets)
    db = rf.Corpus.from_device_ragged(*_device(b, offsets))
    _same_bytes(_saved(db, tmp_path / "devb.rfc"), _saved(hb, tmp_path / "hostb.rfc"), f"{name}: rf_corpus_pack_device")
    assert not db.wide and db.device_bytes == hb.device_bytes
    tb, ob = db.take()
    first = int(offsets[0])
    assert np.array_equal(tb, b[first:]) and np.array_equal(ob, offsets - offsets[0])


@pytest.mark.parametrize("name", CASES)
def test_host_entry_through_the_device_road(name, packed, children, tmp_path):
    work, log = children
    dev_file = open(work / f"{name}.dev.rfc", "rb").read()
    _same_bytes(dev_file, open(work / f"{name}.host.rfc", "rb").read(), f"{name}: RF_DEVICE_PACK_MIN=1 against =0")
    _same_bytes(dev_file, _saved(packed(name)[3], tmp_path / "host.rfc"), f"{name}: the child against this process")
    # the device road was taken: its phase lines (without them this leg would pass on a library that has no device road at all)
    lines = log[name]
    for phase in ("device: u32 upload elems+offsets", "device: u32 symbol histogram", "device: u32 alphabet + id image", "device: lengths + histograms",
                  "device: sort + scatter + tile order"):
        assert phase in lines, (phase, lines)
    overflow = packed(name)[3].alphabet_size()[1]
    assert ("device: u32 raw stream" in lines) == (overflow > 0), lines
    assert "allocate + zero" not in lines  # (no phase of the host packer)


@pytest.mark.parametrize("name", CASES)
def test_take_gives_the_input_back(name, packed):
    data, offsets, _, host, dev = packed(name)
    got, off = dev.take()
    first = int(offsets[0])
    assert got.dtype == np.uint32 and np.array_equal(got, data[first:])
    assert np.array_equal(off, offsets - offsets[0])
    assert dev.alphabet_size() == host.alphabet_size()
    idx = np.array([len(dev) - 1, 0, len(dev) // 2, len(dev) - 1], dtype=np.uint64)
    g1, o1 = dev.take(idx)
    g2, o2 = host.take(idx)
    assert np.array_equal(g1, g2) and np.array_equal(o1, o2)


@pytest.mark.parametrize("name", CASES)
def test_metrics_agree_with_the_host_packed_corpus(name, packed):
    """The existing suite holds the host-packed corpus to the oracle; here the device-packed one must give the same numbers.  The third query carries a
    symbol of the corpus' overflow class: it scans the image translated from the raw stream, so the raw scatter's output is read and not only saved."""
    data, offsets, _, host, dev = packed(name)
    first = int(offsets[0])
    body = data[first:]
    values, counts = np.unique(body, return_counts=True)
    order = np.argsort(-counts.astype(np.int64), kind="stable")
    frequent = values[order[:12]].astype(np.uint32)
    absent = np.uint32(0x2FFFF)
    assert absent not in values
    queries = [np.tile(frequent, 2)[:20], np.concatenate([frequent[:9], [absent], frequent[:7]]).astype(np.uint32)]
    if host.alphabet_size()[1]:
        rare = values[order[-1]]  # the least frequent symbol: one of the overflow class
        queries.append(np.concatenate([frequent[:8], [rare, rare], body[int(offsets[-2]) - first: int(offsets[-2]) - first + 6]]).astype(np.uint32))
    else:
        queries.append(body[int(offsets[5]) - first: int(offsets[6]) - first].astype(np.uint32))
    for q in queries:
        q = np.ascontiguousarray(q, dtype=np.uint32)
        for metric, call in (("levenshtein", "distance_many"), ("indel", "distance_many"), ("jaro_winkler", "similarity_many")):
            bc = getattr(rf.distance, metric).BatchComparator(q)
            a, b = getattr(bc, call)(dev), getattr(bc, call)(host)
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, metric, q[:4])


def _call(fn, d, n_elems, o, n):
    """-> (status, *out, error text); `*out` starts as a sentinel"""
    import torch

    out = C.c_void_p(0x5A5A5A5A)
    st = fn(d.data_ptr(), n_elems, o.data_ptr(), n, d.device.index, torch.cuda.current_stream().cuda_stream, C.byref(out))
    return st, out.value, N.lib().rf_last_error().decode()


@pytest.mark.parametrize("wide", [False, True])
def test_errors_are_invalid_arguments_and_leave_nothing_behind(wide):
    import torch

    data, offsets, _ = make_case("a40")
    if not wide:
        data = as_bytes(data)
    fn = N.lib().rf_corpus_pack_u32_device if wide else N.lib().rf_corpus_pack_device
    name = "rf_corpus_pack_u32_device" if wide else "rf_corpus_pack_device"
    n = len(offsets) - 1
    d, o = _device(data, offsets)
    # decreasing offsets in the middle (first and last stay in order)
    bad = offsets.copy()
    bad[1000], bad[1001] = bad[1001], bad[1000] - np.uint64(1)
    assert bad[1001] < bad[1000]
    _, ob = _device(data, bad)
    st, out, text = _call(fn, d, len(data), ob, n)
    assert st == N.RF_ERR_INVALID_ARG and out == 0x5A5A5A5A and text.startswith(name + ":"), text
    # decreasing from the first to the last: nothing may be launched over such a range
    rev = offsets[::-1].copy()
    _, orv = _device(data, rev)
    st, out, text = _call(fn, d, len(data), orv, n)
    assert st == N.RF_ERR_INVALID_ARG and out == 0x5A5A5A5A and text.startswith(name + ":"), text
    # offsets[n] > n_elems: the buffer is one element shorter than the offsets say
    st, out, text = _call(fn, d, len(data) - 1, o, n)
    assert st == N.RF_ERR_INVALID_ARG and out == 0x5A5A5A5A and text.startswith(name + ":"), text
    if wide:  # the reserved symbol
        poisoned = data.copy()
        poisoned[len(data) // 3] = 0xFFFFFFFF
        dp, _ = _device(poisoned, offsets)
        st, out, text = _call(fn, dp, len(data), o, n)
        assert st == N.RF_ERR_INVALID_ARG and out == 0x5A5A5A5A and "0xFFFFFFFF" in text and text.startswith(name + ":"), text
        with pytest.raises(rf.RfError):
            rf.Corpus.from_device_ragged(dp, o)
    # nothing is left behind on the device.  A failing call that kept its temporaries would keep 0.5 MiB (the length histogram) to 1.1 MiB (+ the symbol counts)
    # per call; after one warm-up round, 24 more rounds of every failing call above may not take 4 MiB of the device's free memory (a leak would take 12 MiB
    # and more; 4 MiB is two of the driver's 2 MiB pages of slack).  The tensors are made before the first reading: torch's allocator is not what is measured.
    failing = [(d, len(data), ob), (d, len(data), orv), (d, len(data) - 1, o)] + ([(dp, len(data), o)] if wide else [])
    before = None
    for rnd in range(25):
        for dd, ne, oo in failing:
            assert _call(fn, dd, ne, oo, n)[0] == N.RF_ERR_INVALID_ARG
        if rnd == 0:
            torch.cuda.synchronize()
            before = torch.cuda.mem_get_info(d.device)[0]
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(d.device)[0]
    print(f"free device memory: {before} before, {after} after {24 * len(failing)} failing calls")
    assert before - after < (4 << 20), (before, after)
    # and the same buffers still pack once the arguments are right
    good = rf.Corpus.from_device_ragged(d, o)
    assert len(good) == n


def test_from_device_ragged_takes_every_documented_dtype_and_refuses_the_rest(tmp_path):
    """uint8 / int32 / uint32 data with int64 / uint64 offsets (the unsigned ones where this torch has them) all give the host packer's corpus; anything else is
    a ValueError before the library is called."""
    import torch

    data, offsets, _ = make_case("a40")
    host = _saved(rf.Corpus.from_ragged_u32(data, offsets), tmp_path / "host.rfc")
    d32, o64 = _device(data, offsets)
    variants = [(d32, o64)]
    if hasattr(torch, "uint32"):
        variants.append((d32.view(torch.uint32), o64))
    if hasattr(torch, "uint64"):
        variants.append((d32, o64.view(torch.uint64)))
    if hasattr(torch, "uint32") and hasattr(torch, "uint64"):
        variants.append((d32.view(torch.uint32), o64.view(torch.uint64)))
    for k, (d, o) in enumerate(variants):
        c = rf.Corpus.from_device_ragged(d, o)
        assert c.wide
        _same_bytes(_saved(c, tmp_path / f"v{k}.rfc"), host, f"{d.dtype} data, {o.dtype} offsets")
    b = as_bytes(data)
    hostb = _saved(rf.Corpus.from_ragged(b, offsets), tmp_path / "hostb.rfc")
    d8, _ = _device(b, offsets)
    for k, o in enumerate([o64] + ([o64.view(torch.uint64)] if hasattr(torch, "uint64") else [])):
        c = rf.Corpus.from_device_ragged(d8, o, stream=torch.cuda.current_stream().cuda_stream)
        assert not c.wide
        _same_bytes(_saved(c, tmp_path / f"b{k}.rfc"), hostb, f"uint8 data, {o.dtype} offsets")
    refused = {
        "int16 data": (d32.view(torch.int16), o64),
        "int64 data": (o64, o64),
        "2-D data": (d32[: 4 * (len(d32) // 4)].view(-1, 4), o64),
        "strided data": (d32[::2], o64),
        "host data": (d32.cpu(), o64),
        "host offsets": (d32, o64.cpu()),
        "int32 offsets": (d32, o64.to(torch.int32)),
        "strided offsets": (d32, o64[::2]),
        "2-D offsets": (d32, o64[: 2 * (len(o64) // 2)].view(-1, 2)),
        "no offsets": (d32, o64[:0]),
    }
    for what, (d, o) in refused.items():
        with pytest.raises(ValueError):
            rf.Corpus.from_device_ragged(d, o)
            pytest.fail(what + " was accepted")


@pytest.mark.parametrize("wide", [False, True])
def test_a_candidate_beyond_65535_symbols_takes_the_host_road(wide, tmp_path):
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 40, size=201)
    lens[77] = 70000
    offsets = np.zeros(len(lens) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens, dtype=np.uint64)
    syms = rng.permutation(np.arange(0x4E00, 0x9FA0))[:600].astype(np.uint32)
    data = _zipf(rng, syms, int(offsets[-1]))
    if not wide:
        data = as_bytes(data)
    host = rf.Corpus.from_ragged_u32(data, offsets) if wide else rf.Corpus.from_ragged(data, offsets)
    dev = rf.Corpus.from_device_ragged(*_device(data, offsets))
    _same_bytes(_saved(dev, tmp_path / "dev.rfc"), _saved(host, tmp_path / "host.rfc"), "one long candidate")
    got, off = dev.take()
    assert np.array_equal(got, data) and np.array_equal(off, offsets)
    assert int(dev.lengths([77])[0]) == 70000
