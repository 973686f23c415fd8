"""rf_corpus_pack_device / rf_corpus_pack_u32_device without a device: both symbols are exported and declared in the header, the Rust declarations and the Python
symbol list, and the three argument errors the header promises "before a device is touched" -- a null out, null offsets with n > 0, a null payload with
elements to read -- are RF_ERR_INVALID_ARG with `*out` untouched and an error text that names the call."""
import ctypes as C
import os
import re

import pytest

import rapidfuzz_rs_amd as rf
from rapidfuzz_rs_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["rf_corpus_pack_device", "rf_corpus_pack_u32_device"]
SENTINEL = 0x5A5A5A5A


@pytest.mark.parametrize("name", CALLS)
def test_symbol_is_exported_and_declared_everywhere(name):
    assert hasattr(N.lib(), name)
    assert name in N.SYMBOLS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rfgpu.h")).read(), flags=re.S)
    m = re.search(r"^rf_status %s\((.*?)\);" % name, hdr, flags=re.S | re.M)
    assert m, f"include/rfgpu.h does not declare {name}"
    names = [re.findall(r"\w+", a)[-1] for a in m.group(1).split(",")]
    assert names == ["d_bytes" if name == "rf_corpus_pack_device" else "d_elems", "n_elems", "d_offsets", "n", "device", "stream", "out"]
    sys_rs = open(os.path.join(ROOT, "rust", "rapidfuzz-gpu", "src", "sys.rs")).read()
    m = re.search(r"pub fn %s\((.*?)\) -> RfStatus;" % name, sys_rs)
    assert m, f"sys.rs does not declare {name}"
    assert [a.split(":")[0].strip() for a in m.group(1).split(",")] == names
    assert hasattr(rf.Corpus, "from_device_ragged")
    facade = open(os.path.join(ROOT, "include", "rapidfuzz_amd.hpp")).read()
    assert "from_device_ragged" in facade and name + "(" in facade


class _Call:
    """Valid-looking arguments; the stand-ins for device memory are addresses the call may not reach: each case must be refused before a device is touched."""

    def __init__(self, name):
        self.fn = getattr(N.lib(), name)
        self.mem = (C.c_uint8 * 4096)()
        self.payload = C.addressof(self.mem)
        self.offsets = C.addressof(self.mem) + 2048
        self.n_elems = 100
        self.n = 3
        self.out = C.c_void_p(SENTINEL)
        self.outp = C.byref(self.out)

    def run(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)
        return self.fn(self.payload, self.n_elems, self.offsets, self.n, 0, None, self.outp)


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("what", ["out", "offsets", "payload"])
def test_argument_errors_answer_before_a_device_is_touched(name, what):
    c = _Call(name)
    if what == "out":
        st = c.run(outp=None)
    elif what == "offsets":
        st = c.run(offsets=None)
    else:
        st = c.run(payload=None)
    assert st == N.RF_ERR_INVALID_ARG
    assert c.out.value == SENTINEL  # *out untouched
    text = N.lib().rf_last_error().decode()
    assert text.startswith(name + ":"), text
