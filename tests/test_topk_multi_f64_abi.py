"""rf_topk_multi_f64 without a device: the symbol is exported and declared in the header, the Rust declarations, the Python symbol list and
the C++ facade, and its argument checks answer before the corpus is looked at or a device is touched (include/rfgpu.h says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 4


def test_symbol_is_exported_and_declared_in_all_three_places():
    assert hasattr(N.lib(), "rf_topk_multi_f64")
    assert "rf_topk_multi_f64" in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status rf_topk_multi_f64\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_topk_multi_f64"
    names = [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")]
    assert names == ["cs", "q", "corpus", "op", "args", "k", "index_base", "out_score", "out_index", "out_count", "stream"]
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn rf_topk_multi_f64\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_topk_multi_f64"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == names
    assert hasattr(rf.fuzz.RatioBatchComparator, "topk_multi")
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "normalized_similarity_topk_multi" in facade and "normalized_distance_topk_multi" in facade and "rf_topk_multi_f64(" in facade
    wrapper = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "metric.rs")).read()
    assert "rf_topk_multi_f64(" in wrapper and "normalized_similarity_topk_multi" in wrapper


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-in for the corpus is zeroed memory that none of
    the calls below may reach: every one of them has to be refused (or, q == 0, answered) before the corpus is looked at."""

    def __init__(self, metrics=("levenshtein", "indel")):
        self.cs = [getattr(rf.distance, m).BatchComparator(b"kitten") for m in metrics]
        self.hs = (C.c_void_p * len(self.cs))(*[c._h for c in self.cs])
        self.q = len(self.cs)
        self.corpus_mem = (C.c_uint8 * 8192)()
        self.corpus = C.addressof(self.corpus_mem)
        self.args = rf.Args().to_c(True)
        self.argp = C.byref(self.args)
        self.k = K
        self.score = np.full((self.q, K), 77.0, dtype=np.float64)
        self.index = np.full((self.q, K), 77, dtype=np.uint64)
        self.count = np.full(self.q, 77, dtype=np.uint32)
        self.op = N.OP_NORMALIZED_SIMILARITY

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        score = self.score.ctypes.data if isinstance(self.score, np.ndarray) else self.score
        index = self.index.ctypes.data if isinstance(self.index, np.ndarray) else self.index
        count = self.count.ctypes.data if isinstance(self.count, np.ndarray) else self.count
        return N.lib().rf_topk_multi_f64(self.hs, self.q, self.corpus, self.op, self.argp, self.k, 0, score, index, count, None)


@pytest.mark.parametrize("what", ["cs", "corpus", "args", "comparator", "out_count"])
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
    else:
        st = c.run(count=None)
    assert st == N.RF_ERR_INVALID_ARG
    assert N.lib().rf_last_error()  # (a reason is recorded)
    if what != "out_count":
        assert (c.count == 77).all() and (c.score == 77).all()  # nothing was written


def test_k_zero_is_an_invalid_argument():
    assert _Call().run(k=0) == N.RF_ERR_INVALID_ARG


@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
@pytest.mark.parametrize("metric", ["levenshtein", "indel", "lcs_seq", "osa", "damerau_levenshtein"])
def test_the_u32_valued_ops_of_a_usize_metric_are_invalid_arguments(metric, op):
    c = _Call(metrics=("jaro", metric))
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert b"rf_topk_multi_u32" in N.lib().rf_last_error()  # (the message names the call that serves them)
    assert (c.count == 77).all() and (c.score == 77).all() and (c.index == 77).all()


def test_a_distance_op_of_the_ratio_is_an_invalid_argument():
    c = _Call()
    ratio = rf.fuzz.RatioBatchComparator(b"kitten")
    for op in (N.OP_DISTANCE, N.OP_NORMALIZED_DISTANCE):
        assert c.run(hs=(C.c_void_p * 2)(c.cs[0]._h, ratio._h), op=op) == N.RF_ERR_INVALID_ARG
    assert (c.count == 77).all() and (c.score == 77).all()


def test_an_unknown_op_is_an_invalid_argument():
    assert _Call().run(op=4) == N.RF_ERR_INVALID_ARG


def test_no_queries_is_ok_and_writes_nothing():
    c = _Call()
    assert c.run(q=0) == N.RF_OK
    assert (c.count == 77).all() and (c.score == 77).all() and (c.index == 77).all()
