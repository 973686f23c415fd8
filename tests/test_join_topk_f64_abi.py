"""rf_join_topk_f64 without a device: the symbol is exported and declared -- argument names in order -- in the header, the Rust declarations and the Python symbol
list, it is used by the C++ facade, the Rust crate and the Python classes (the usize metrics, fuzz.RatioBatchComparator, jaro / jaro_winkler), and its argument
checks answer before either corpus is looked at or a device is touched, with nothing written (include/rfgpu.h says so).  The decode both f64 top-k calls share
(decode_norm_keys, rf_host.hpp) is written once; tests/test_norm_key.py goes on checking the key and its inverse themselves."""
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
ND, NS = N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_symbol_is_exported_and_declared_everywhere():
    assert hasattr(N.lib(), "rf_join_topk_f64")
    assert "rf_join_topk_f64" in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "rfgpu.h"), flags=re.S)
    m = re.search(r"^rf_status rf_join_topk_f64\((.*?)\);", hdr, flags=re.S | re.M)
    assert m, "include/rfgpu.h does not declare rf_join_topk_f64"
    assert [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")] == ARGS
    assert "double *out_score" in m.group(1)
    assert hdr.index("rf_status rf_join_topk_u32(") < hdr.index("rf_status rf_join_topk_f64(")  # (the section follows the u32 call)
    sys_rs = _read("rust", "rapidfuzz-gpu", "src", "sys.rs")
    m = re.search(r"pub fn rf_join_topk_f64\((.*?)\) -> RfStatus;", sys_rs)
    assert m, "sys.rs does not declare rf_join_topk_f64"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == ARGS
    corpus_rs = _read("rust", "rapidfuzz-gpu", "src", "corpus.rs")
    assert "pub fn join_topk_f64(" in corpus_rs and "rf_join_topk_f64(" in corpus_rs
    facade = _read("include", "rapidfuzz_amd.hpp")
    assert "normalized_distance_join_topk" in facade and "normalized_similarity_join_topk" in facade and "rf_join_topk_f64(" in facade
    for name in ("levenshtein", "indel", "lcs_seq", "osa", "damerau_levenshtein", "hamming", "prefix", "postfix", "jaro", "jaro_winkler"):
        assert hasattr(getattr(rf.distance, name).BatchComparator, "join_topk_f64"), name
    assert hasattr(rf.fuzz.RatioBatchComparator, "join_topk_f64")


def test_the_header_names_the_call_where_it_named_the_hole():
    header = _read("include", "rfgpu.h")
    assert "an rf_join_topk_f64" not in header  # (the u32 call's out-of-scope list no longer begins with it)
    at = header.index("join, top-k by f64 score")
    section = header[at: header.index("rf_status rf_join_topk_f64(", at)]
    for part in ("a wider key for maxima beyond 65535", "an early-out variant", "device-resident output", "a multi-GPU form", "a fused road for `char` corpora",
                 "[rf plan] join_topk_f64: m=.. k=.. batches=.. groups=.. units=.. per_query=.."):
        assert part in section, part


def test_the_decode_is_written_once_and_both_calls_use_it():
    host = _read("rapidfuzz_rs_amd", "csrc", "rf_host.hpp")
    assert host.count("inline uint32_t decode_norm_keys(") == 1
    srcs = {f: _read("rapidfuzz_rs_amd", "csrc", f) for f in ("rf_api_topk_multi.hip", "rf_api_join.hip")}
    for f, src in srcs.items():
        assert "decode_norm_keys(" in src, f
        assert "(double)r.a / (double)r.b" not in src, f  # (the division is written in the one decode)
    assert host.count("(double)r.a / (double)r.b") == 1
    # the shared pieces are parametrized, not copied: one definition each
    join = srcs["rf_api_join.hip"]
    for fn in ("rf_status check_join_topk_args(", "rf_status join_rows(", "rf_status join_lengths(", "rf_status join_plan_rows(", "struct JoinBatches", "rf_status join_topk_device(",
               "rf_status join_topk_per_query(", "rf_status join_topk_call("):
        assert join.count(fn) == 1, fn
    assert join.count('env_on("RF_JOIN")') == 1 and join.count('env_int("RF_JOIN_BATCH"') == 1 and join.count('env_int("RF_JOIN_TOPK_UNITS"') == 1


class _Call:
    """One call with valid-looking arguments; a test replaces what it is about.  The stand-ins for the two corpora are zeroed memory that none of the calls
    below may reach: every one of them has to be refused (or, m == 0, answered) before a corpus is looked at."""

    def __init__(self):
        self.queries_mem, self.corpus_mem = (C.c_uint8 * 8192)(), (C.c_uint8 * 8192)()
        self.queries, self.corpus = C.addressof(self.queries_mem), C.addressof(self.corpus_mem)
        self.args = rf.Args().to_c(True)  # (no cutoff: none is needed)
        self.argp = C.byref(self.args)
        self.idx = np.array([0, 1, 2], dtype=np.uint64)
        self.m = 3
        self.k = K
        self.sc = np.full(3 * K, 77.0, dtype=np.float64)
        self.oi = np.full(3 * K, 77, dtype=np.uint64)
        self.cnt = np.full(3, 77, dtype=np.uint32)
        self.metric, self.op, self.flags = N.LEVENSHTEIN, NS, 0

    def run(self, **kw):
        for name, v in kw.items():
            setattr(self, name, v)
        p = lambda a: a.ctypes.data if isinstance(a, np.ndarray) else a  # noqa: E731
        return N.lib().rf_join_topk_f64(self.metric, self.queries, p(self.idx), self.m, self.corpus, self.op, self.argp, self.flags, self.k, 0, p(self.sc), p(self.oi),
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


@pytest.mark.parametrize("metric", [N.LEVENSHTEIN, N.INDEL, N.LCS_SEQ, N.OSA, N.DAMERAU_LEVENSHTEIN, N.HAMMING, N.PREFIX, N.POSTFIX])
@pytest.mark.parametrize("op", [N.OP_DISTANCE, N.OP_SIMILARITY])
def test_distance_and_similarity_of_a_usize_metric_are_invalid_arguments(metric, op):
    c = _Call()
    assert c.run(metric=metric, op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("op", [N.OP_DISTANCE, ND])
def test_a_distance_op_of_fuzz_ratio_is_an_invalid_argument(op):
    c = _Call()
    assert c.run(metric=N.FUZZ_RATIO, op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric", [N.LEVENSHTEIN, N.FUZZ_RATIO, N.JARO])
@pytest.mark.parametrize("op", [17, -1])
def test_unknown_ops_are_invalid_arguments(metric, op):
    c = _Call()
    assert c.run(metric=metric, op=op) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric", [99, -1])
def test_unknown_metrics_are_invalid_arguments(metric):
    c = _Call()
    assert c.run(metric=metric) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("flags", [N.JOIN_UPPER, N.JOIN_UPPER | N.JOIN_NO_SELF, 4, 0x80000000])
def test_upper_and_unknown_flag_bits_are_invalid_arguments(flags):
    c = _Call()
    assert c.run(flags=flags) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


def test_the_argument_errors_come_before_the_rule_for_no_queries():
    c = _Call()
    assert c.run(m=0, k=0) == N.RF_ERR_INVALID_ARG
    assert c.run(m=0, k=K, flags=N.JOIN_UPPER) == N.RF_ERR_INVALID_ARG
    assert c.run(m=0, k=K, flags=0, op=N.OP_DISTANCE) == N.RF_ERR_INVALID_ARG
    assert c.untouched()


@pytest.mark.parametrize("metric,op", [(N.LEVENSHTEIN, ND), (N.LEVENSHTEIN, NS), (N.OSA, NS), (N.HAMMING, ND), (N.FUZZ_RATIO, N.OP_SIMILARITY), (N.FUZZ_RATIO, NS),
                                       (N.JARO, N.OP_DISTANCE), (N.JARO, N.OP_SIMILARITY), (N.JARO_WINKLER, ND), (N.JARO_WINKLER, NS)])
def test_no_queries_is_ok_and_writes_nothing_for_every_accepted_pair(metric, op):
    c = _Call()
    assert c.run(m=0, metric=metric, op=op) == N.RF_OK
    assert c.run(m=0, flags=N.JOIN_NO_SELF) == N.RF_OK
    assert c.untouched()
    # ... even with null outputs
    assert c.run(m=0, sc=None, oi=None, cnt=None) == N.RF_OK


@pytest.mark.parametrize("what", ["sc", "oi", "cnt"])
def test_a_null_output_with_queries_is_an_invalid_argument(what):
    c = _Call()
    assert c.run(**{what: None}) == N.RF_ERR_INVALID_ARG  # (still before a corpus is looked at: the stand-ins are zeroed memory)
    assert c.untouched()


def test_the_python_methods_keep_to_their_score_types():
    lev, jaro = rf.distance.levenshtein.BatchComparator, rf.distance.jaro.BatchComparator
    with pytest.raises(ValueError):
        lev.join_topk_f64(None, None, 1, N.OP_DISTANCE)
    with pytest.raises(ValueError):
        lev.join_topk_f64(None, None, 1, N.OP_SIMILARITY)
    for k in (-1, 2**32):  # (checked before either corpus is touched: it would not fit the call's uint32_t)
        with pytest.raises(ValueError):
            lev.join_topk_f64(None, None, k)
    # join_topk itself keeps its behaviour
    with pytest.raises(ValueError):
        jaro.join_topk(None, None, 1, N.OP_SIMILARITY)
    with pytest.raises(ValueError):
        lev.join_topk(None, None, 1, ND)
    with pytest.raises(ValueError):
        rf.fuzz.RatioBatchComparator.join_topk(None, None, 1, N.OP_SIMILARITY)
