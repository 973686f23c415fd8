"""rf_join_f64 without a device (the counterpart of tests/test_join_abi.py): the symbol is exported and declared in the header, the Rust declarations and the
Python symbol list, it is used by the C++ facade, the Rust crate and the Python classes, both joins read their two switches through the one knob reader, and
its argument checks answer before either corpus is looked at or a device is touched, with nothing written (include/rfgpu.h says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 4
ARGS = ["metric", "queries", "query_indices", "m", "corpus", "op", "args", "flags", "query_base", "index_base", "capacity", "out_query", "out_index", "out_score",
        "out_count", "order", "stream"]
TYPES = ["rf_metric", "const rf_corpus *", "const uint64_t *", "uint64_t", "const rf_corpus *", "rf_op", "const rf_args *", "uint32_t", "uint64_t", "uint64_t", "uint64_t",
         "uint64_t *", "uint64_t *", "double *", "uint64_t *", "rf_join_order", "void *"]
USIZE = ("levenshtein", "indel", "lcs_seq", "osa", "damerau_levenshtein", "hamming", "prefix", "postfix")
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY


def test_symbol_is_exported_and_declared_everywhere():
    assert hasattr(N.lib(), "rf_join_f64")
    assert "rf_join_f64" in N.SYMBOLS
    assert len(N.lib().rf_join_f64.argtypes) == len(ARGS)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status rf_join_f64\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_join_f64"
    params = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [re.findall(r"\w+", a)[-1] for a in params] == ARGS
    assert [re.sub(r"\w+$", "", a).strip() for a in params] == TYPES
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn rf_join_f64\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_join_f64"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == ARGS
    assert "out_score: *mut f64" in m.group(1)
    corpus_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "corpus.rs")).read()
    assert "pub fn join_f64(" in corpus_rs and "rf_join_f64(" in corpus_rs
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "struct JoinTripleF64" in facade and "normalized_distance_join" in facade and "normalized_similarity_join" in facade and "rf_join_f64(" in facade
    for name in USIZE + ("jaro", "jaro_winkler"):
        assert hasattr(getattr(rf.distance, name).BatchComparator, "join_f64"), name
    assert hasattr(rf.fuzz.RatioBatchComparator, "join_f64")


def test_both_joins_read_their_switches_through_the_one_knob_reader():
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    for knob in (r"RF_JOIN +1 ", r"RF_JOIN_BATCH +16384 "):
        line = re.search(r"^ \*   " + knob + ".*$", header, flags=re.M)
        assert line and "rf_join_u32" in line.group(0) and "rf_join_f64" in line.group(0)
    src = open(os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc", "rf_api_join.hip")).read()
    assert src.count('env_on("RF_JOIN")') == 1 and src.count('env_int("RF_JOIN_BATCH"') == 1 and "getenv" not in src  # (one reader each, for both calls)
    assert "rf_status rf_join_u32(" in src and "rf_status rf_join_f64(" in src  # (... which live in the one file)


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-ins for the two corpora are zeroed memory that none of the calls
    below may reach: every one of them has to be refused (or, m == 0, answered) before a corpus is looked at."""

    def __init__(self):
        self.queries_mem, self.corpus_mem = (C.c_uint8 * 8192)(), (C.c_uint8 * 8192)()
        self.queries, self.corpus = C.addressof(self.queries_mem), C.addressof(self.corpus_mem)
        self.args = rf.Args().score_cutoff(0.9).to_c(True)
        self.argp = C.byref(self.args)
        self.idx = np.array([0, 1, 2], dtype=np.uint64)
        self.m = 3
        self.capacity = CAP
        self.oq = np.full(CAP, 77, dtype=np.uint64)
        self.oi = np.full(CAP, 77, dtype=np.uint64)
        self.sc = np.full(CAP, 77.0, dtype=np.float64)
        self.count = np.full(1, 77, dtype=np.uint64)
        self.metric, self.op, self.order, self.flags = N.LEVENSHTEIN, NS, N.JOIN_BY_QUERY, 0

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        p = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a  # noqa: E731
        count = self.count.ctypes.data_as(C.POINTER(C.c_uint64)) if isinstance(self.count, np.ndarray) else self.count
        return N.lib().rf_join_f64(self.metric, self.queries, p(self.idx), self.m, self.corpus, self.op, self.argp, self.flags, 0, 0, self.capacity, p(self.oq), p(self.oi),
                                   p(self.sc), count, self.order, None)

    def untouched(self):
        return all((a == 77).all() for a in (self.oq, self.oi, self.sc, self.count) if isinstance(a, np.ndarray))


def test_a_valid_looking_call_is_what_the_others_vary():
    """(the base call differs from every refused one below in the one thing that test names: m == 0 of it is answered, so its other arguments pass)"""
    c = _Call()
    assert c.run(m=0) == N.RF_OK and c.untouched()


@pytest.mark.parametrize("what", ["queries", "corpus", "args", "out_count", "out_query", "out_index", "out_score"])
def test_null_pointers_are_invalid_arguments(what):
    c = _Call()
    st = c.run(**{{"queries": "queries", "corpus": "corpus", "args": "argp", "out_count": "count", "out_query": "oq", "out_index": "oi", "out_score": "sc"}[what]: None})
    assert st == N.RF_ERR_INVALID_ARG
    assert N.lib().rf_last_error()  # (a reason is recorded)
    assert c.untouched()  # nothing was written


@pytest.mark.parametrize("order", [-1, 2, 99])
def test_an_unknown_order_is_an_invalid_argument(order):
    c = _Call()
    assert c.run(order=order) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("flags", [2, 3, 0x80000000])
def test_an_unknown_flag_bit_is_an_invalid_argument(flags):
    c = _Call()
    assert c.run(flags=flags) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric", [8, 12, 99, -1])
def test_an_unknown_metric_is_an_invalid_argument(metric):
    assert metric not in (N.LEVENSHTEIN, N.INDEL, N.LCS_SEQ, N.OSA, N.DAMERAU_LEVENSHTEIN, N.HAMMING, N.PREFIX, N.POSTFIX, N.JARO, N.JARO_WINKLER, N.FUZZ_RATIO)
    c = _Call()
    assert c.run(metric=metric) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("op", [17, -1])
def test_an_unknown_op_is_an_invalid_argument(op):
    for metric in (N.LEVENSHTEIN, N.JARO, N.FUZZ_RATIO):
        c = _Call()
        assert c.run(metric=metric, op=op) == N.RF_ERR_INVALID_ARG
        assert c.untouched()


@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
def test_the_u32_valued_ops_of_levenshtein_are_invalid_arguments_that_point_to_the_u32_call(op):
    c = _Call()
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert b"rf_join_u32" in N.lib().rf_last_error()
    assert c.untouched()


@pytest.mark.parametrize("op", [ND, N.OP_DISTANCE])
def test_a_distance_op_of_fuzz_ratio_is_an_invalid_argument(op):
    c = _Call()
    assert c.run(metric=N.FUZZ_RATIO, op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric,op", [(N.LEVENSHTEIN, NS), (N.LEVENSHTEIN, ND), (N.FUZZ_RATIO, N.OP_SIMILARITY), (N.JARO_WINKLER, N.OP_SIMILARITY)])
def test_a_nan_cutoff_is_refused(metric, op):
    c = _Call()
    c.args = rf.Args().to_c(True)
    assert np.isnan(c.args.cutoff_f64)
    assert c.run(metric=metric, op=op, argp=C.byref(c.args)) == N.RF_ERR_INVALID_ARG
    assert b"cutoff" in N.lib().rf_last_error()
    assert c.untouched()


@pytest.mark.parametrize("metric,op", [(N.LEVENSHTEIN, NS), (N.OSA, ND), (N.FUZZ_RATIO, N.OP_SIMILARITY), (N.FUZZ_RATIO, NS), (N.JARO, N.OP_DISTANCE), (N.JARO_WINKLER, NS)])
def test_no_queries_is_ok_and_writes_nothing(metric, op):
    c = _Call()
    assert c.run(metric=metric, op=op, m=0) == N.RF_OK
    assert c.untouched()
    # a pure count of no queries: the arrays may be NULL
    assert c.run(m=0, capacity=0, oq=None, oi=None, sc=None) == N.RF_OK
    assert (c.count == 77).all()


def test_the_python_method_refuses_u32_valued_ops_on_a_usize_class():
    for name in USIZE:
        for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
            with pytest.raises(ValueError):
                getattr(rf.distance, name).BatchComparator.join_f64(None, None, op, score_cutoff=0.9)
    # ... and join keeps refusing what join_f64 serves
    with pytest.raises(ValueError):
        rf.fuzz.RatioBatchComparator.join(None, None, N.OP_SIMILARITY, score_cutoff=1)
