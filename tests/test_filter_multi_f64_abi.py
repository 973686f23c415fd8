"""rf_filter_multi_f64 without a device: the symbol is exported and declared in the header, the Rust declarations and the Python symbol
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
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY


def test_symbol_is_exported_and_declared_in_all_three_places():
    assert hasattr(N.lib(), "rf_filter_multi_f64")
    assert "rf_filter_multi_f64" in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status rf_filter_multi_f64\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_filter_multi_f64"
    names = [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")]
    assert names == ["cs", "q", "corpus", "op", "args", "index_base", "capacity", "out_index", "out_score", "out_count", "order", "stream"]
    assert "double *out_score" in m.group(1)
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn rf_filter_multi_f64\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_filter_multi_f64"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == names
    assert "out_score: *mut f64" in m.group(1)
    metric_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "metric.rs")).read()
    assert "rf_filter_multi_f64(" in metric_rs
    assert "fn normalized_distance_filter_multi" in metric_rs and "fn normalized_similarity_filter_multi" in metric_rs
    assert hasattr(rf.fuzz.RatioBatchComparator, "filter_multi")
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "normalized_distance_filter_multi" in facade and "normalized_similarity_filter_multi" in facade and "rf_filter_multi_f64(" in facade
    assert re.search(r"\bfilter_multi_f64\(", facade)
    ratio = facade[facade.index("class RatioBatchComparator"):]
    assert "similarity_filter_multi" in ratio


def test_the_header_places_it_below_the_u32_form_and_the_switch_names_both_calls():
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    assert header.index("rf_status rf_filter_multi_u32(") < header.index("rf_status rf_filter_multi_f64(") < header.index("rf_status rf_topk_u32(")
    m = re.search(r"^ \*   RF_FILTER_MULTI +1 +(.*)$", header, flags=re.M)
    assert m and "rf_filter_multi_u32" in m.group(1) and "_f64" in m.group(1)


def test_the_documents_no_longer_say_the_f64_form_is_missing():
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    assert "rf_filter_f64 per query), device-resident" not in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "no `rf_filter_multi_f64`" not in design and "5.7.2" in design
    for doc in ("README.md", "INTEGRATION.md"):
        assert "filter_multi_f64" in open(os.path.join(ROOT, doc)).read() or "normalized_similarity_filter_multi" in open(os.path.join(ROOT, doc)).read(), doc


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-in for the corpus is zeroed memory that none of
    the calls below may reach: every one of them has to be refused (or, q == 0, answered) before the corpus is looked at."""

    def __init__(self, metrics=("levenshtein", "indel")):
        self.cs = [getattr(rf.distance, m).BatchComparator(b"kitten") for m in metrics]
        self.hs = (C.c_void_p * len(self.cs))(*[c._h for c in self.cs])
        self.q = len(self.cs)
        self.corpus_mem = (C.c_uint8 * 8192)()
        self.corpus = C.addressof(self.corpus_mem)
        self.args = rf.Args().score_cutoff(0.9).to_c(True)
        self.argp = C.byref(self.args)
        self.capacity = CAP
        self.index = np.full((self.q, CAP), 77, dtype=np.uint64)
        self.score = np.full((self.q, CAP), 77.0, dtype=np.float64)
        self.count = np.full(self.q, 77, dtype=np.uint64)
        self.op = NS
        self.order = N.FILTER_BY_INDEX

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        index = self.index.ctypes.data if isinstance(self.index, np.ndarray) else self.index
        score = self.score.ctypes.data if isinstance(self.score, np.ndarray) else self.score
        count = self.count.ctypes.data if isinstance(self.count, np.ndarray) else self.count
        return N.lib().rf_filter_multi_f64(self.hs, self.q, self.corpus, self.op, self.argp, 0, self.capacity, index, score, count, self.order, None)

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


@pytest.mark.parametrize("op", [-1, 4, 17])
def test_an_unknown_op_is_an_invalid_argument(op):
    c = _Call()
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
def test_the_u32_valued_ops_of_a_usize_metric_point_to_the_u32_call(op):
    c = _Call()
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert b"rf_filter_multi_u32" in N.lib().rf_last_error()
    assert c.untouched()
    # ... also when only a later member is a usize metric
    c = _Call(metrics=("jaro", "levenshtein"))
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("op", [N.OP_DISTANCE, ND])
def test_a_distance_op_of_the_ratio_is_an_invalid_argument(op):
    c = _Call(metrics=("jaro", "jaro_winkler"))  # (members that accept every op: the ratio alone is what is refused)
    ratio = rf.fuzz.RatioBatchComparator(b"kitten")
    assert c.run(hs=(C.c_void_p * 2)(c.cs[0]._h, ratio._h), op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_no_queries_is_ok_and_writes_nothing():
    c = _Call()
    assert c.run(q=0) == N.RF_OK
    assert c.untouched()
    # a pure count of no queries: the row arrays may be NULL
    assert c.run(q=0, capacity=0, index=None, score=None) == N.RF_OK
    assert (c.count == 77).all()


@pytest.mark.parametrize("metric", ["jaro", "jaro_winkler"])
@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY, ND, NS])
def test_jaro_comparators_pass_the_argument_checks(metric, op):
    """every op of jaro / jaro_winkler is accepted.  The comparator loop is the last argument check, so a list that is refused only for a LATER
    member -- a null one -- has passed the jaro member through it: the reason names the null comparator, not the metric or the op."""
    c = _Call(metrics=(metric, "levenshtein"))
    assert c.run(hs=(C.c_void_p * 2)(c.cs[0]._h, None), op=op) == N.RF_ERR_INVALID_ARG
    assert b"null comparator" in N.lib().rf_last_error()
    assert c.untouched()


def test_the_ratio_with_its_similarity_ops_passes_the_argument_checks():
    ratio = rf.fuzz.RatioBatchComparator(b"kitten")
    for op in (N.OP_SIMILARITY, NS):
        c = _Call()
        assert c.run(hs=(C.c_void_p * 2)(ratio._h, None), op=op) == N.RF_ERR_INVALID_ARG
        assert b"null comparator" in N.lib().rf_last_error()
        assert c.untouched()
