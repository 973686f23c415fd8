"""rf_host_layout_candidate: the host-only inverse of rf_corpus_layout_host, through ctypes -- every index of every shape the take tests share
(tests/take_shapes.py) comes back as it went in; a capacity shorter than the row writes that many bytes and still reports the length; NULL / 0 is a sizing call;
an index >= n, a null layout / out_len and a null buffer with a capacity are RF_ERR_INVALID_ARG with nothing written."""
import ctypes as C

import numpy as np
import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

import take_shapes


class _Layout:
    def __init__(self, candidates):
        data, offsets = rf.corpus.ragged(candidates)
        self.lay = N.RfHostLayout()
        N.check(N.lib().rf_corpus_layout_host(data.ctypes.data, offsets.ctypes.data, len(candidates), C.byref(self.lay)))

    def candidate(self, index, capacity=512, buf=None):
        buf = np.full(max(capacity, 1) + 8, 0xA5, dtype=np.uint8) if buf is None else buf
        ln = C.c_uint32(0xDEAD)
        st = N.lib().rf_host_layout_candidate(C.byref(self.lay), index, buf.ctypes.data if capacity else None, capacity, C.byref(ln))
        return st, ln.value, buf

    def __del__(self):
        N.lib().rf_host_layout_free(C.byref(self.lay))


@pytest.fixture(scope="module", params=take_shapes.NAMES)
def case(request):
    cands = take_shapes.shape(request.param)
    return cands, _Layout(cands)


def test_every_index_comes_back(case):
    cands, lay = case
    assert lay.lay.n == len(cands)
    assert bool(lay.lay.identity) == (len({len(c) for c in cands}) == 1)
    for i, want in enumerate(cands):
        st, ln, buf = lay.candidate(i)
        assert st == N.RF_OK and ln == len(want) and buf[:ln].tobytes() == want, i
        assert (buf[ln:] == 0xA5).all(), i  # nothing past the candidate's end


def test_short_capacity_writes_that_much_and_reports_the_length(case):
    cands, lay = case
    for i in range(0, len(cands), 13):
        want = cands[i]
        for cap in {0, 1, len(want) // 2, max(len(want) - 1, 0)}:
            st, ln, buf = lay.candidate(i, capacity=cap)
            assert st == N.RF_OK and ln == len(want)
            k = min(cap, len(want))
            assert buf[:k].tobytes() == want[:k] and (buf[k:] == 0xA5).all()


def test_invalid_arguments_write_nothing(case):
    cands, lay = case
    n = len(cands)
    for index in (n, n + 1, 2**32, 2**64 - 1):
        st, ln, buf = lay.candidate(index)
        assert st == N.RF_ERR_INVALID_ARG and ln == 0xDEAD and (buf == 0xA5).all()
    ln = C.c_uint32(0xDEAD)
    buf = np.full(64, 0xA5, dtype=np.uint8)
    L = N.lib()
    assert L.rf_host_layout_candidate(None, 0, buf.ctypes.data, 64, C.byref(ln)) == N.RF_ERR_INVALID_ARG
    assert L.rf_host_layout_candidate(C.byref(lay.lay), 0, buf.ctypes.data, 64, None) == N.RF_ERR_INVALID_ARG
    assert L.rf_host_layout_candidate(C.byref(lay.lay), 0, None, 64, C.byref(ln)) == N.RF_ERR_INVALID_ARG
    assert ln.value == 0xDEAD and (buf == 0xA5).all()
    assert L.rf_last_error()
