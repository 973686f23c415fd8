"""rf_join_topk_u32 without a device: the symbol is exported and declared -- argument names in order -- in the header, the Rust declarations and the Python symbol
list, it is used by the C++ facade, the Rust crate and the eight Python classes, its flag and its switch are in the header, and its argument checks answer before
either corpus is looked at or a device is touched, with nothing written (include/rfgpu.h says so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 3
ARGS = ["metric", "queries", "query_indices", "m", "corpus", "op", "args", "flags", "k", "index_base", "out_score", "out_index", "out_count", "stream"]


def test_symbol_is_exported_and_declared_everywhere():
    assert hasattr(N.lib(), "rf_join_topk_u32")
    assert "rf_join_topk_u32" in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status rf_join_topk_u32\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_join_topk_u32"
    assert [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")] == ARGS
    assert re.search(r"^#define RF_JOIN_NO_SELF 2u", hdr, flags=re.M)
    assert hdr.index("rf_status rf_join_f64(") < hdr.index("rf_status rf_join_topk_u32(")  # (the section follows the f64 join)
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn rf_join_topk_u32\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_join_topk_u32"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == ARGS
    assert "pub const RF_JOIN_NO_SELF: u32 = 0x2;" in sys_rs
    corpus_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "corpus.rs")).read()
    assert "pub fn join_topk(" in corpus_rs and "rf_join_topk_u32(" in corpus_rs and "RF_JOIN_NO_SELF" in corpus_rs
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "distance_join_topk" in facade and "similarity_join_topk" in facade and "rf_join_topk_u32(" in facade
    for name in ("levenshtein", "indel", "lcs_seq", "osa", "damerau_levenshtein", "hamming", "prefix", "postfix"):
        assert hasattr(getattr(rf.distance, name).BatchComparator, "join_topk"), name
    assert (N.JOIN_UPPER, N.JOIN_NO_SELF) == (1, 2)
    make = open(os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc", "Makefile")).read()
    assert "rf_join_topk.hip" in make and "rf_api_join.hip" in make and "rf_join_plan.hpp" in make


def test_the_switch_is_in_the_environment_table_and_read_through_the_knob_reader():
    header = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
    assert re.search(r"^ \*   RF_JOIN_TOPK_UNITS +0 \(auto\) ", header, flags=re.M)
    src = open(os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc", "rf_api_join.hip")).read()
    assert 'env_int("RF_JOIN_TOPK_UNITS"' in src and "getenv" not in src
    # the new call reads RF_JOIN and RF_JOIN_BATCH through the readers that were there: one reader each
    assert src.count('env_on("RF_JOIN")') == 1 and src.count('env_int("RF_JOIN_BATCH"') == 1
    kernel = open(os.path.join(ROOT, "rapidfuzz_rs_amd", "csrc", "rf_join_topk.hip")).read()
    assert "env_" not in kernel and "getenv" not in kernel


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-ins for the two corpora are zeroed memory that none of the calls
    below may reach: every one of them has to be refused (or, m == 0, answered) before a corpus is looked at."""

    def __init__(self):
        self.queries_mem, self.corpus_mem = (C.c_uint8 * 8192)(), (C.c_uint8 * 8192)()
        self.queries, self.corpus = C.addressof(self.queries_mem), C.addressof(self.corpus_mem)
        self.args = rf.Args().to_c(False)  # (no cutoff: none is needed)
        self.argp = C.byref(self.args)
        self.idx = np.array([0, 1, 2], dtype=np.uint64)
        self.m = 3
        self.k = K
        self.sc = np.full(3 * K, 77, dtype=np.uint32)
        self.oi = np.full(3 * K, 77, dtype=np.uint64)
        self.cnt = np.full(3, 77, dtype=np.uint32)
        self.metric, self.op, self.flags = N.LEVENSHTEIN, N.OP_DISTANCE, 0

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        p = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a  # noqa: E731
        return N.lib().rf_join_topk_u32(self.metric, self.queries, p(self.idx), self.m, self.corpus, self.op, self.argp, self.flags, self.k, 0, p(self.sc), p(self.oi),
                                        p(self.cnt), None)

    def untouched(self):
        return all((a == 77).all() for a in (self.sc, self.oi, self.cnt) if isinstance(a, np.ndarray))


@pytest.mark.parametrize("what", ["queries", "corpus", "args"])
def test_null_handles_and_args_are_invalid_arguments(what):
    c = _Call()
    st = c.run(**{{"queries": "queries", "corpus": "corpus", "args": "argp"}[what]: None})
    assert st == N.RF_ERR_INVALID_ARG
    assert N.lib().rf_last_error()  # (a reason is recorded)
    assert c.untouched()


def test_k_zero_is_an_invalid_argument():
    c = _Call()
    assert c.run(k=0) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("op", [N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY, 17, -1])
def test_other_ops_are_invalid_arguments(op):
    c = _Call()
    assert c.run(op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("flags", [N.JOIN_UPPER, N.JOIN_UPPER | N.JOIN_NO_SELF, 4, 0x80000000])
def test_upper_and_unknown_flag_bits_are_invalid_arguments(flags):
    c = _Call()
    assert c.run(flags=flags) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric", [N.JARO, N.JARO_WINKLER, N.FUZZ_RATIO, 99, -1])
def test_f64_valued_and_unknown_metrics_are_invalid_arguments(metric):
    c = _Call()
    assert c.run(metric=metric) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_the_argument_errors_come_before_the_rule_for_no_queries():
    c = _Call()
    assert c.run(m=0, k=0) == N.RF_ERR_INVALID_ARG
    assert c.run(m=0, k=K, flags=N.JOIN_UPPER) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_no_queries_is_ok_and_writes_nothing():
    c = _Call()
    assert c.run(m=0) == N.RF_OK
    assert c.run(m=0, flags=N.JOIN_NO_SELF) == N.RF_OK
    assert c.untouched()
    # ... even with null outputs
    assert c.run(m=0, sc=None, oi=None, cnt=None) == N.RF_OK


@pytest.mark.parametrize("what", ["sc", "oi", "cnt"])
def test_a_null_output_with_queries_is_an_invalid_argument(what):
    c = _Call()
    assert c.run(**{what: None}) == N.RF_ERR_INVALID_ARG  # (still before a corpus is looked at: the stand-ins are zeroed memory)
    assert c.untouched()


def test_the_joins_keep_refusing_the_new_flag():
    q, c = (C.c_uint8 * 8192)(), (C.c_uint8 * 8192)()
    cnt = C.c_uint64(77)
    for fn, op, args in ((N.lib().rf_join_u32, N.OP_DISTANCE, rf.Args().score_cutoff(2).to_c(False)),
                         (N.lib().rf_join_f64, N.OP_NORMALIZED_DISTANCE, rf.Args().score_cutoff(0.5).to_c(True))):
        assert fn(N.LEVENSHTEIN, C.addressof(q), None, 3, C.addressof(c), op, C.byref(args), N.JOIN_NO_SELF, 0, 0, 0, None, None, None, C.byref(cnt), N.JOIN_BY_QUERY,
                  None) == N.RF_ERR_INVALID_ARG
        assert cnt.value == 77


def test_the_python_method_refuses_float_classes_and_normalized_ops():
    with pytest.raises(ValueError):
        rf.distance.jaro.BatchComparator.join_topk(None, None, 1, N.OP_SIMILARITY)
    with pytest.raises(ValueError):
        rf.distance.levenshtein.BatchComparator.join_topk(None, None, 1, N.OP_NORMALIZED_DISTANCE)
    for k in (-1, 2**32):  # (checked before either corpus is touched: it would not fit the call's uint32_t)
        with pytest.raises(ValueError):
            rf.distance.levenshtein.BatchComparator.join_topk(None, None, k)
