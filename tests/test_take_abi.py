"""rf_corpus_is_wide / rf_corpus_lengths / rf_corpus_take / rf_corpus_take_u32 without a device: the symbols are exported and declared in the header (with the
parameter names the issue gives), the Rust declarations and the Python symbol list, they are used by the C++ facade and the Rust wrapper, and every argument
check that does not need the corpus' contents answers before the corpus is looked at or a device is touched, with nothing written (include/rfgpu.h says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {
    "rf_corpus_is_wide": ["c"],
    "rf_corpus_lengths": ["c", "indices", "m", "index_base", "out_len", "stream"],
    "rf_corpus_take": ["c", "indices", "m", "index_base", "out_bytes", "capacity", "out_offsets", "out_mem", "stream"],
    "rf_corpus_take_u32": ["c", "indices", "m", "index_base", "out_elems", "capacity", "out_offsets", "out_mem", "stream"],
}


@pytest.mark.parametrize("name", list(PARAMS))
def test_symbol_is_exported_and_declared_in_all_three_places(name):
    assert hasattr(N.lib(), name)
    assert name in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^(?:rf_status|int) +%s\((.*?)\);" % name, hdr, flags=re.S | re.M)
    assert m, f"include/rfgpu.h does not declare {name}"
    names = [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")]
    assert names == PARAMS[name]
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\) -> (?:RfStatus|c_int);" % name, sys_rs)
    assert m, f"sys.rs does not declare {name}"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == names
    assert name + "(" in open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "corpus.rs")).read()
    assert name + "(" in open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read() or name + "," in open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()


def test_the_upper_layers_offer_the_call():
    for attr in ("take", "lengths", "to_list", "__getitem__", "wide"):
        assert hasattr(rf.Corpus, attr), attr
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    for item in ("std::vector<std::string> take(", "std::vector<std::u32string> take_u32(", "std::vector<uint32_t> lengths("):
        assert item in facade, item
    wrapper = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "corpus.rs")).read()
    assert "pub fn take(" in wrapper and "pub fn take_chars(" in wrapper
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    scope = header[header.index("candidates read back out of the packed corpus"):header.index("rf_status rf_corpus_take_u32(")]
    assert "for c in corpus" in scope  # names the reference item
    out_of_scope = scope[scope.index("Out of scope:"):]
    for item in ("device-resident `indices` or offsets", "FILE that is not loaded", "multi-GPU"):
        assert item in out_of_scope, item


SENTINEL = 0x77


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-in for the corpus is zeroed memory: a corpus of no candidates that owns
    nothing, so every index is out of range, and nothing else of it may be reached."""

    def __init__(self, fn):
        self.fn = fn
        self.corpus_mem = (C.c_uint8 * 16384)()
        self.corpus = C.addressof(self.corpus_mem)
        self.indices = np.array([5, 6, 7], dtype=np.uint64)
        self.m = 3
        self.index_base = 0
        self.capacity = 64
        self.payload = np.full(64, SENTINEL, dtype=np.uint32)
        self.offsets = np.full(8, SENTINEL, dtype=np.uint64)
        self.lens = np.full(8, SENTINEL, dtype=np.uint32)
        self.out_mem = N.MEM_HOST

    @staticmethod
    def _ptr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        L = N.lib()
        if self.fn == "rf_corpus_lengths":
            return L.rf_corpus_lengths(self.corpus, self._ptr(self.indices), self.m, self.index_base, self._ptr(self.lens), None)
        return getattr(L, self.fn)(self.corpus, self._ptr(self.indices), self.m, self.index_base, self._ptr(self.payload), self.capacity, self._ptr(self.offsets),
                                   self.out_mem, None)

    def untouched(self):
        return all((a == SENTINEL).all() for a in (self.payload, self.offsets, self.lens) if isinstance(a, np.ndarray))


TAKES = ["rf_corpus_take", "rf_corpus_take_u32"]
ALL = TAKES + ["rf_corpus_lengths"]


@pytest.mark.parametrize("fn", ALL)
def test_a_null_corpus_is_an_invalid_argument(fn):
    c = _Call(fn)
    assert c.run(corpus=None) == N.RF_ERR_INVALID_ARG
    assert N.lib().rf_last_error() and c.untouched()
    assert N.lib().rf_corpus_is_wide(None) == 0


@pytest.mark.parametrize("fn", ALL)
def test_a_null_offsets_or_lengths_array_is_an_invalid_argument(fn):
    c = _Call(fn)
    # (no indices: m == n == 0 would otherwise be answered RF_OK)
    assert c.run(offsets=None, lens=None, indices=None, m=0) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("fn", TAKES)
def test_a_null_payload_with_a_capacity_is_an_invalid_argument(fn):
    c = _Call(fn)
    assert c.run(payload=None, indices=None, m=0) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("fn", ALL)
def test_no_indices_must_ask_for_every_candidate(fn):
    c = _Call(fn)
    assert c.run(indices=None, m=3) == N.RF_ERR_INVALID_ARG  # (the stand-in has 0 candidates)
    assert c.untouched()


@pytest.mark.parametrize("fn", TAKES)
@pytest.mark.parametrize("out_mem", [-1, 2, 99])
def test_an_unknown_out_mem_is_an_invalid_argument(fn, out_mem):
    c = _Call(fn)
    assert c.run(out_mem=out_mem, indices=None, m=0) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("fn", ALL)
def test_an_index_outside_the_corpus_is_an_invalid_argument(fn):
    c = _Call(fn)
    assert c.run() == N.RF_ERR_INVALID_ARG  # every index is >= n = 0
    assert c.run(index_base=6) == N.RF_ERR_INVALID_ARG  # 5 lies below the base
    assert c.untouched()


@pytest.mark.parametrize("fn", TAKES)
def test_no_rows_is_ok_and_writes_one_offset(fn):
    c = _Call(fn)
    assert c.run(m=0) == N.RF_OK
    assert c.offsets[0] == 0 and (c.offsets[1:] == SENTINEL).all() and (c.payload == SENTINEL).all()
    c = _Call(fn)
    assert c.run(m=0, indices=None, payload=None, capacity=0) == N.RF_OK  # every candidate of an empty corpus, as a sizing call
    assert c.offsets[0] == 0 and (c.offsets[1:] == SENTINEL).all()


def test_no_lengths_is_ok_and_writes_nothing():
    c = _Call("rf_corpus_lengths")
    assert c.run(m=0) == N.RF_OK and c.untouched()
