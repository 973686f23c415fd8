"""rf_filter_multi_u32 without a device: the symbol is exported and declared in the header, the Rust declarations and the Python symbol
list, it is used by the C++ facade, and its argument checks answer before the corpus is looked at or a device is touched, with nothing
written (include/rfgpu.h says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4


def test_symbol_is_exported_and_declared_in_all_three_places():
    assert hasattr(N.lib(), "rf_filter_multi_u32")
    assert "rf_filter_multi_u32" in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status rf_filter_multi_u32\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_filter_multi_u32"
    names = [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")]
    assert names == ["cs", "q", "corpus", "op", "args", "index_base", "capacity", "out_index", "out_score", "out_count", "order", "stream"]
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn rf_filter_multi_u32\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_filter_multi_u32"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == names
    assert "rf_filter_multi_u32(" in open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "metric.rs")).read()
    assert hasattr(rf.distance.levenshtein.BatchComparator, "filter_multi")
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "distance_filter_multi" in facade and "similarity_filter_multi" in facade and "rf_filter_multi_u32(" in facade


def test_the_switch_is_in_the_environment_table():
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    assert re.search(r"^ \*   RF_FILTER_MULTI +1 ", header, flags=re.M)


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-in for the corpus is zeroed memory that none of
    the calls below may reach: every one of them has to be refused (or, q == 0, answered) before the corpus is looked at."""

    def __init__(self, metrics=("levenshtein", "indel")):
        self.cs = [getattr(rf.distance, m).BatchComparator(b"kitten") for m in metrics]
        self.hs = (C.c_void_p * len(self.cs))(*[c._h for c in self.cs])
        self.q = len(self.cs)
        self.corpus_mem = (C.c_uint8 * 8192)()
        self.corpus = C.addressof(self.corpus_mem)
        self.args = rf.Args().score_cutoff(2).to_c(False)
        self.argp = C.byref(self.args)
        self.capacity = CAP
        self.index = np.full((self.q, CAP), 77, dtype=np.uint64)
        self.score = np.full((self.q, CAP), 77, dtype=np.uint32)
        self.count = np.full(self.q, 77, dtype=np.uint64)
        self.op = N.OP_DISTANCE
        self.order = N.FILTER_BY_INDEX

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        index = self.index.ctypes.data if isinstance(self.index, np.ndarray) else self.index
        score = self.score.ctypes.data if isinstance(self.score, np.ndarray) else self.score
        count = self.count.ctypes.data if isinstance(self.count, np.ndarray) else self.count
        return N.lib().rf_filter_multi_u32(self.hs, self.q, self.corpus, self.op, self.argp, 0, self.capacity, index, score, count, self.order, None)

    def untouched(self):
        return all((a == 77).all() for a in (self.index, self.score, self.count) if isinstance(a, np.ndarray))


@pytest.mark.parametrize("what", ["cs", "corpus", "args", "comparator", "out_count", "out_index", "out_score"])
def test_null_pointers_are_invalid_arguments(what):
    c = _Call()
    if what == "cs":
        st = c.run(hs=None)
    elif what == "corpus":
        st = c.run(corpus=None)
    elif what == "args":
        st = c.run(argp=None)
    elif what == "comparator":
        st = c.run(hs=(C.c_void_p * 2)(c.cs[0]._h, None))
    elif what == "out_count":
        st = c.run(count=None)
    elif what == "out_index":
        st = c.run(index=None)
    else:
        st = c.run(score=None)
    assert st == N.RF_ERR_INVALID_ARG
    assert N.lib().rf_last_error()  # (a reason is recorded)
    assert c.untouched()  # nothing was written


@pytest.mark.parametrize("order", [-1, 3, 99])
def test_an_unknown_order_is_an_invalid_argument(order):
    c = _Call()
    assert c.run(order=order) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric", ["jaro", "jaro_winkler"])
def test_f64_valued_metrics_are_invalid_arguments(metric):
    c = _Call(metrics=("levenshtein", metric))
    assert c.run() == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_ratio_comparator_is_an_invalid_argument():
    c = _Call()
    ratio = rf.fuzz.RatioBatchComparator(b"kitten")
    assert c.run(hs=(C.c_void_p * 2)(c.cs[0]._h, ratio._h)) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_other_ops_are_invalid_arguments():
    for op in (N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY, 17):
        c = _Call()
        assert c.run(op=op) == N.RF_ERR_INVALID_ARG
        assert c.untouched()


def test_no_queries_is_ok_and_writes_nothing():
    c = _Call()
    assert c.run(q=0) == N.RF_OK
    assert c.untouched()
    # a pure count of no queries: the row arrays may be NULL
    assert c.run(q=0, capacity=0, index=None, score=None) == N.RF_OK
    assert (c.count == 77).all()
