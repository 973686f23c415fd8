"""The host side of the hamming / prefix / postfix surface: the metric ids (9, 10, 11 -- 8 stays no metric), the pad flag and the two encodings of
hamming's Err(DifferentLengthArgs) in header, Python mirror and Rust binding, the op / output-type rules decided before a device is touched, and the
Python modules.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "rfgpu.h")).read()
SYS = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
IDS = {"HAMMING": 9, "PREFIX": 10, "POSTFIX": 11}
assert {name: getattr(N, name) for name in IDS} == IDS  # (the Python mirror's constants: everything below is about these metrics)


def _new(metric, q=b"hamming"):
    h = C.c_void_p()
    buf = (C.c_uint8 * max(1, len(q))).from_buffer_copy(q or b"\0")
    return N.lib().rf_comparator_new(metric, buf, len(q), C.byref(h)), h


def _new_u32(metric, q=(104, 0x9999, 109)):
    h = C.c_void_p()
    arr = np.asarray(q, dtype=np.uint32)
    return N.lib().rf_comparator_new_u32(metric, arr.ctypes.data, len(arr), C.byref(h)), h


@pytest.mark.parametrize("name", sorted(IDS))
def test_the_ids_are_accepted_by_new_new_u32_and_clone(name):
    L, metric = N.lib(), IDS[name]
    assert getattr(N, name) == metric
    for status, h in (_new(metric), _new_u32(metric), _new(metric, b"")):
        assert status == N.RF_OK and h.value
        assert L.rf_comparator_metric(h) == metric
        cl = C.c_void_p()
        assert L.rf_comparator_clone(h, C.byref(cl)) == N.RF_OK and L.rf_comparator_metric(cl) == metric
        assert L.rf_comparator_query_len(cl) == L.rf_comparator_query_len(h)
        n = C.c_size_t(77)
        assert not L.rf_comparator_pm(h, C.byref(n))  # no pattern-match table in these modules of the reference
        L.rf_comparator_free(cl)
        L.rf_comparator_free(h)


@pytest.mark.parametrize("metric", [8, 12, 13, -1])
def test_ids_outside_the_metrics_are_refused(metric):
    for status, h in (_new(metric), _new_u32(metric)):
        assert status == N.RF_ERR_INVALID_ARG and not h.value


def test_flag_and_encodings_agree_between_header_python_and_rust():
    def hdr(name):
        return int(re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+)" % name, HDR).group(1), 16)

    def rust(name):
        return int(re.search(r"pub const %s: \w+ = (0x[0-9A-Fa-f_]+);" % name, SYS).group(1).replace("_", ""), 16)

    assert hdr("RF_FLAG_HAMMING_PAD") == N.FLAG_HAMMING_PAD == rust("RF_FLAG_HAMMING_PAD") == 0x4
    assert hdr("RF_DIFFERENT_LENGTH_U32") == N.DIFFERENT_LENGTH_U32 == rust("RF_DIFFERENT_LENGTH_U32") == 0xFFFFFFFE
    assert hdr("RF_DIFFERENT_LENGTH_F64_BITS") == N.DIFFERENT_LENGTH_F64_BITS == rust("RF_DIFFERENT_LENGTH_F64_BITS") == 0x7FF8000000000001
    assert hdr("RF_NONE_F64_BITS") == N.NONE_F64_BITS == rust("RF_NONE_F64_BITS") == 0x7FF8000000000000
    for name, v in IDS.items():
        assert re.search(r"\bRF_%s\s*=\s*%d\b" % (name, v), HDR) and re.search(r"pub const RF_%s: c_int = %d;" % (name, v), SYS)
    assert not re.search(r"RF_\w+\s*=\s*8\b", re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)) and "8 is NOT a metric" in HDR
    # the two NaNs: both NaN to isnan, different by bits; the flag collides with no other
    both = np.array([N.NONE_F64_BITS, N.DIFFERENT_LENGTH_F64_BITS], dtype=np.uint64).view(np.float64)
    assert np.isnan(both).all() and N.NONE_F64_BITS != N.DIFFERENT_LENGTH_F64_BITS
    assert len({N.FLAG_RATIO_INDEL_NORMALIZATION, N.FLAG_SLOT_ORDER, N.FLAG_HAMMING_PAD}) == 3
    assert N.DIFFERENT_LENGTH_U32 != N.NONE_U32
    # rf_args keeps its layout
    assert C.sizeof(N.RfArgs) == 72 and N.RfArgs.flags.offset == 64


@pytest.mark.parametrize("name", sorted(IDS))
def test_wrong_op_and_output_type_pairs_are_refused_before_a_device_is_touched(name):
    """The stand-in for the corpus is zeroed memory -- what an empty byte corpus looks like to the planner (no candidates, no lengths, no device buffers), as
    in tests/test_filter_multi_abi.py: an empty corpus never selects a device, and plan() still decides."""
    L = N.lib()
    mod = getattr(rf.distance, name.lower())
    bc = mod.BatchComparator(b"prefix")
    mem = (C.c_uint8 * 65536)()

    class corpus:
        _h = C.addressof(mem)

    a = N.RfArgs()
    L.rf_args_default(C.byref(a))
    out = (C.c_double * 4)()
    for op in (N.OP_NORMALIZED_DISTANCE, N.OP_NORMALIZED_SIMILARITY):
        assert L.rf_many_u32(bc._h, corpus._h, op, C.byref(a), out, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
        assert L.rf_many_f64(bc._h, corpus._h, op, C.byref(a), out, N.MEM_HOST, None) == N.RF_OK
    for op in (N.OP_DISTANCE, N.OP_SIMILARITY):
        assert L.rf_many_f64(bc._h, corpus._h, op, C.byref(a), out, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG
        assert name.lower() in L.rf_last_error().decode()
        assert L.rf_many_u32(bc._h, corpus._h, op, C.byref(a), out, N.MEM_HOST, None) == N.RF_OK
    assert L.rf_many_u32(bc._h, corpus._h, 4, C.byref(a), out, N.MEM_HOST, None) == N.RF_ERR_INVALID_ARG


def test_rf_one_reports_different_lengths_before_a_device_is_touched():
    L = N.lib()
    bc = rf.distance.hamming.BatchComparator(b"ham")
    a = N.RfArgs()
    L.rf_args_default(C.byref(a))
    s2 = (C.c_uint8 * 7).from_buffer_copy(b"hamming")
    v32, vf, some = C.c_uint32(5), C.c_double(5.0), C.c_int(5)
    assert L.rf_one_u32(bc._h, s2, 7, N.OP_DISTANCE, C.byref(a), 0, C.byref(v32), C.byref(some)) == N.RF_ERR_INVALID_ARG
    assert L.rf_last_error().decode() == "Differing length arguments provided"
    assert L.rf_one_f64(bc._h, s2, 7, N.OP_NORMALIZED_DISTANCE, C.byref(a), 0, C.byref(vf), C.byref(some)) == N.RF_ERR_INVALID_ARG
    assert L.rf_last_error().decode() == "Differing length arguments provided"
    assert (v32.value, vf.value, some.value) == (5, 5.0, 5)  # nothing written


def test_python_modules_and_args():
    assert {"hamming", "prefix", "postfix"} <= set(rf.distance.__all__)
    for name, metric in (("hamming", 9), ("prefix", 10), ("postfix", 11)):
        mod = getattr(rf.distance, name)
        assert mod.BatchComparator.METRIC == metric and not mod.BatchComparator.FLOAT
        for fn in ("distance", "similarity", "normalized_distance", "normalized_similarity", "distance_with_args"):
            assert callable(getattr(mod, fn))
    a = rf.distance.hamming.Args()
    assert a.to_c(False).flags == 0
    assert a.pad().to_c(False).flags == N.FLAG_HAMMING_PAD and a.pad(True).pad(False).to_c(False).flags == 0
    assert a.pad().slot_order().to_c(False).flags == N.FLAG_HAMMING_PAD | N.FLAG_SLOT_ORDER
    assert a.pad().score_cutoff(3).to_c(False).cutoff_usize == 3


def test_the_probe_keeps_refusing_the_new_metrics():
    out = C.c_double()
    for metric in IDS.values():
        assert N.lib().rf_probe_issue_rate(metric, 64, 0, 0, 0, C.byref(out)) == N.RF_ERR_UNSUPPORTED
